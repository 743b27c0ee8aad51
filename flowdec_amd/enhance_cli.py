"""Command-line driver equivalent to the reference's `enhance.py`.

    python -m flowdec_amd.enhance_cli --ckpt flowdec_75m.ckpt --files noisy_dir/ --outdir out/ --N 3 --solver midpoint [--rtf]
    python -m flowdec_amd.enhance_cli --ckpt scoredec.ckpt --files noisy_dir/ --outdir out/ --N 30 --predictor reverse_diffusion --corrector ald --snr 0.5

Same arguments and file conventions as the reference (enhance.py:24-49): `--files` is a directory of *.wav, a file list
(one path per line, or `clean ---> noisy` / `clean,noisy` pair lines, enhance.py:146-164) or, with `--single-file`, one
wav; files longer than 30 s are skipped (:115,:139); `--rtf` writes `path,runtime,filetime,rtf` rows (:94,:135) with
rtf = runtime / filetime like the reference.

Model class: like `EnhancementModel.load_from_checkpoint` (enhance.py:66) the driver runs the class the checkpoint names in
`hyper_parameters.model._target_` -- FlowModel, ScoreModel (config/baseline_scoredec_75s.yaml) or RegressionModel
(config/baseline_regression_75s.yaml); a checkpoint that names none (no hyper_parameters, a bare state_dict) is a FlowModel, and
`--model {flow,score,regression}` overrides the checkpoint.  `--predictor`, `--corrector`, `--snr` and `--N` reach the score model's
sampler (a FlowModel ignores the first three); `--solver` is the flow model's (the two baselines ignore it, as in the reference).  All
three classes run in ragged batches; the regression model draws no noise and ignores `--seed` / `--rng`.

Checkpoints: a Lightning `.ckpt` (dict with `_pl_ema_state_dict` and/or `state_dict`, optionally `hyper_parameters`
holding the resolved config: callbacks/ema.py:201-215, model.py:100,119) or a bare state_dict (flowdec_amd/checkpoint.py).  `--ema`
(default) selects the EMA weights exactly like `demo.ipynb` cell 2.

Non-48 kHz input is resampled with a restatement of torchaudio.functional.resample(..., lowpass_filter_width=64)
(enhance.py:118; torchaudio itself is not a dependency): `sinc_resample_kernel` / `resample` of flowdec_amd/audio.py.

Batching (round 6): the reference enhances one file per call (enhance.py:96-137).  This driver reads the lengths first, buckets the
files by the frame count their spectrogram pads to (T_pad, util/other.py:25-52) and runs up to `--batch-files` files of a bucket as
ONE ragged native call (`enhance_batch` of the model class -> fd_enhance_ragged / fd_score_enhance_ragged / fd_regression_enhance_ragged): every file's waveform is bit-identical to the one-file call,
the GPU sees a batch.  With `--seed S` file i of the work list draws its noise from its own generator seeded S + i, so the result
of a file does not depend on the batching (`--batch-files 1` = the reference's loop); with `--rng native` the noise is the library's
own, generated on the GPU from `flowdec_amd.noise.clip_seed(S, i)` (no collisions between (S, i + 1) and (S + 1, i)).  Under `--rtf` a batch is timed as a whole and
its time is split over its files in proportion to their duration (every file of a batch gets the batch's rtf).

Adaptive solvers: `--solver dopri5` / `tsit5` accept or reject a step on one error ratio over the whole native call, so by default
(`--step-control batch`) a flow model runs them one file per call.  `--step-control clip` gives every file its own step controller
(`FlowModel.enhance_batch(step_control='clip')` -> fd_ode_solve_adaptive_clips): the files are bucketed and batched like everything
else, and every file's waveform is still the one-file result, bit for bit.

ODE sampler of a score model: `--sampler ode` (`--ode-rtol`, `--ode-atol`, default 1e-5) integrates the probability-flow ODE on the
device under scipy RK45's step-size rule instead of running the predictor-corrector sampler: the buckets go through
`ScoreModel.enhance_ode_batch` (one step controller per file, so a file's waveform does not depend on its batch), `--predictor`,
`--corrector` and `--snr` are ignored with one printed line, and every file's NFE is printed (`rtfs.csv` has no column for it).
`--sampler pc` (the default) changes nothing.

Length limit: the reference skips files longer than 30 s; so does this driver by default, in every precision.  `--max-seconds S`
moves that limit: the kernels address images of any length that fits in device memory (a 180 s clip in bf16 is one call), and
what remains is the device memory itself.  A file whose workspace (`fd_enhance_workspace_bytes`) does not fit in the free device
memory is skipped WITH a message, like a file over a precision's limit (`PRECISION_MAX_SECONDS`, where a precision with a shorter
reach would say so): the exit status is then 3.

Long files: `--chunk-seconds S` (default: off) lifts both limits for a FlowModel with `--rng native`.  A file with more samples than a row
of S seconds holds (S seconds in STFT frames, rounded down to a multiple of 64, at least 64: `longform.chunk_row_frames`) is not
subject to the length rule; it runs through `FlowModel.enhance_long` -- overlapping rows of that many frames in a workspace that does not
grow with the file (halos of 256 frames, or a quarter of the row if that is less), seeded with the file's `clip_seed(SEED, i)` -- one file per call, with its own `--rtf` row and a message that
names the limits it is exempt from.  `--batch-files` rows run per call; if their workspace does not fit, the file is skipped with a message like any other
file over memory.  Every other file takes
the paths above and gives the same bytes as without the flag.

Several GPUs: `--gpus N` runs the corpus on the first N devices of the node.  The launching process never opens a GPU: it plans the work
list once, writes it as a JSON manifest into --outdir (so that a rank that starts late does not take its siblings' outputs for existing
ones) and starts N fresh worker processes of this module, all at once.  Worker r loads the checkpoint on cuda:r, makes the SAME batch plan
as a one-process run (the plan does not depend on N), costs every batch (`batch_cost`), takes `dist.balance(costs, N)[r]` and runs those
batches with exactly the one-process code, in plan order.  The launcher relays the workers' output prefixed `[rank r]`, merges their
`rtfs{suffix}.rank{r}.csv` parts into the one `rtfs{suffix}.csv` in plan order -- the rows and the order of a one-process run --, writes
`triples_list{suffix}.txt`, sums the counts (exit status 3 as before) and removes the parts and the manifest.  File i is seeded from
(SEED, i) whatever rank and batch it lands in, so every output file has the bytes of the one-process run.  A worker that ends with an
ordinary error leaves the others to finish; the launcher then exits non-zero, names the rank and keeps the part files (a rerun with
--skip-existing completes what is missing).  A worker that ends by a signal, an abort or a segmentation fault makes the launcher stop the
others: nothing more is started on a GPU that may have faulted.  `--share-gpu` puts all ranks on cuda:0 (at most 8): a test aid for
one-GPU boxes, not a speed-up.  The split is static (no work stealing): that is what makes rtfs.csv reproducible.

Evaluation: `--eval` (pair lists only, default off; without it nothing changes) scores the `triples_list{suffix}.txt` the run has just
written -- after the merge in the launcher of a --gpus N run -- with `flowdec_amd.eval_cli` on one GPU: SI-SDR / SI-SIR / SI-SAR and
LogSpecMSE per triple into `metrics{suffix}.csv` beside the list.  The files are scored as they were written to disk, as the reference's
evaluation scores them (flowdec/eval/metrics.py).  `--eval-estoi` (with --eval) passes `--estoi` on: a fifth column, ESTOI;
`--eval-spectral` passes `--spectral` on: two last columns, the multi-scale STFT and mel distances; `--eval-align MS` passes `--align MS` on:
the triples are aligned in time within +-MS milliseconds before they are scored, two last columns `lag_x_hat` and `lag_y`;
`--eval-align-frac` and `--eval-align-polarity` (with --eval-align MS) pass `--align-frac` and `--align-polarity` on: sub-sample delays,
and an inverted polarity undone with two further last columns `pol_x_hat` and `pol_y`; `--eval-loudness` and `--eval-match-loudness` pass
`--loudness` and `--match-loudness` on: the integrated loudness (BS.1770) of the three signals in three columns behind the metrics, and
x_hat and y scaled to x's loudness before they are scored; `--eval-ssnr` passes `--ssnr` on: two columns behind the other metrics, the
reference's `fwSSNR` and `SSNR` (the frequency-weighted segmental SNR and the segmental SNR); `--eval-loudness-range` and
`--eval-true-peak` pass `--loudness-range` and `--true-peak` on: the loudness range (EBU Tech 3342) and the true peak (BS.1770-4 Annex 2)
of the three signals, three columns each behind the `lufs_*` columns.

Level of the written files: `--target-lufs VALUE|input` and `--peak-ceiling DBTP` (default off; without them nothing changes and nothing is
measured).  A post-filter should not change the level of what it filters, and a delivery specification caps the true peak (EBU R 128: -23
LUFS and -1 dBTP; the codec package this project restates normalises to -16 LUFS in front of its file path).  The finished output of every
file -- the stitched output of a --chunk-seconds file included -- is measured on the GPU after, and outside, the region --rtf times: its
integrated loudness and its true peak (loudness.file_level_batch; the level of a file is one number: where a waveform has several channels
their K-weighted energies are added with unit weights and gated once, and the true peak is the largest of theirs -- the models here take
one channel, so today every file has one).  ONE gain per file follows (loudness.output_gain):
target - lufs, where the target is VALUE or, with `input`, the loudness of the file's own input measured the same way, capped so that
dbtp + gain does not exceed the ceiling (default -1.0 with --target-lufs) -- a gain cap, not a limiter.  --peak-ceiling alone asks for 0
dB: a file over the ceiling is turned down to it, the others stay.  Every sample gets ONE float32 multiply before the file is written.  A
file without a finite level (under 400 ms, silent) is written as it is, with a warning.  `loudness{suffix}.csv` beside `rtfs{suffix}.csv`
holds name, lufs, dbtp (both of the output BEFORE the gain), gain_db (nan: none) and limited (1: the ceiling capped the gain) for every
file written in this run, in plan order; a --gpus N run merges its workers' parts into the same bytes.  A measurement is the same bits in
any batch and on any rank, so the outputs are those of a one-process run.
"""
import argparse
import collections
import contextlib
import glob
import json
import os
import re
import subprocess
import sys
import threading
import time
from dataclasses import dataclass
from typing import List, Optional, Tuple

import torch

from . import eval_cli, longform, loudness
from .audio import (load_wav, read_list, resample, resample_to, resampled_length, save_wav, sinc_resample_kernel,  # noqa: F401
                    wav_info)
from .batching import padded_frames_of, plan_clip_batches
from .checkpoint import load_from_checkpoint, model_from_checkpoint  # noqa: F401
from .dist import balance
from .model import FlowModel, RegressionModel, ScoreModel, WorkspaceTooLarge
from .noise import clip_seed

MAX_SECONDS = 30.0  # enhance.py:115
SHARE_GPU_MAX_RANKS = 8   # --share-gpu: worker processes on the one GPU
PRECISION_MAX_SECONDS = {}   # precision -> clip length it can take, if shorter than --max-seconds (none: every mode takes any length that fits in memory)
PRECISION_NOTE = {   # printed at start-up so that a log says which arithmetic produced the files
    "bf16": "bf16 storage and MFMA operands, f32 accumulation; ~2e-2 relative waveform error vs the fp32 reference on random weights",
    "mixed": "f32 residual stream, bf16 MFMA operands; ~1.3e-2",
    "bf16x3": "f32 storage, split-bf16 operands (3 MFMAs per product): meets the fp32 tolerances (~3e-5)",
    "fp32": "exact f32 MFMA (~6e-6); slowest",
}


# ------------------------------------------------------------------------------------------------
# main loop
# ------------------------------------------------------------------------------------------------
def target_lufs_arg(text: str):
    """--target-lufs: `input` or a finite number of LUFS."""
    if text.strip().lower() == "input":
        return "input"
    try:
        value = float(text)
    except ValueError:
        value = float("nan")
    if value != value or value in (float("inf"), float("-inf")):
        raise argparse.ArgumentTypeError(f"{text!r} is neither a finite number of LUFS nor `input`")
    return value


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="Enhance wav files with a FlowDec postfilter (or its ScoreDec / regression baselines) on MI355X")
    p.add_argument("--ckpt", type=str, required=True)
    p.add_argument("--files", type=str, required=True)
    p.add_argument("--outdir", type=str, required=True)
    p.add_argument("--N", type=int, required=True)
    p.add_argument("--single-file", action="store_true")
    p.add_argument("--exclude-files-matching", type=str, required=False)
    p.add_argument("--predictor", type=str, default="reverse_diffusion", choices=["reverse_diffusion", "euler_maruyama"])   # score model only
    p.add_argument("--corrector", type=str, default="ald", choices=["ald", "none"])
    p.add_argument("--snr", type=float, default=0.5)
    p.add_argument("--sampler", type=str, default="pc", choices=["pc", "ode"],
                   help="score model only.  pc: the predictor-corrector sampler (--predictor, --corrector, --snr).  ode: the probability-flow ODE "
                        "under scipy RK45's step-size rule on the device (ScoreModel.enhance_ode_batch: one step controller per file, so every "
                        "file's waveform does not depend on its batch); --predictor, --corrector and --snr are then ignored")
    p.add_argument("--ode-rtol", type=float, default=1e-5, help="--sampler ode: relative tolerance of the adaptive solve")
    p.add_argument("--ode-atol", type=float, default=1e-5, help="--sampler ode: absolute tolerance of the adaptive solve")
    p.add_argument("--solver", type=str, default="midpoint")   # flow model only
    p.add_argument("--step-control", type=str, default="batch", choices=["batch", "clip"],
                   help="adaptive --solver (dopri5, tsit5) of a flow model: batch = one step controller per native call, so files run one per "
                        "call; clip = one controller per file, so files of one T_pad bucket share a call (--batch-files) and every file's "
                        "waveform is the one-file result, bit for bit")
    p.add_argument("--model", type=str, default="auto", choices=["auto", "flow", "score", "regression"],
                   help="auto: the class the checkpoint names (hyper_parameters.model._target_; none named: flow); the others override it")
    p.add_argument("--device", type=str, default="cuda:0")
    p.add_argument("--ema", type=lambda s: str(s).lower() not in ("0", "false", "no"), default=True)
    p.add_argument("--skip-existing", type=lambda s: str(s).lower() not in ("0", "false", "no"), default=True)
    p.add_argument("--i-min", type=int, default=None)
    p.add_argument("--i-max", type=int, default=None)
    p.add_argument("--rtf", action="store_true")
    p.add_argument("--precision", type=str, default="bf16", choices=["bf16", "fp32", "mixed", "bf16x3"])
    p.add_argument("--seed", type=int, default=None, help="file i of the work list draws its initial noise from a generator seeded SEED + i "
                                                          "(default: nondeterministic like the reference)")
    p.add_argument("--rng", type=str, default="torch", choices=["torch", "native"],
                   help="torch: the noise comes from torch generators (see --seed); native: the library draws it on the GPU, file i of the work "
                        "list from flowdec_amd.noise.clip_seed(SEED, i) (without --seed one seed is drawn from the OS and printed)")
    p.add_argument("--max-seconds", type=float, default=MAX_SECONDS,
                   help="files longer than this are skipped (default: the reference's %g s); longer clips are limited by device memory only" % MAX_SECONDS)
    p.add_argument("--chunk-seconds", type=float, default=None,
                   help="files longer than a row of this many seconds (in STFT frames, rounded down to a multiple of 64) are enhanced in overlapping "
                        "rows of that length, in fixed device memory, instead of being skipped by --max-seconds; needs --rng native and a flow "
                        "model (default: off)")
    p.add_argument("--batch-files", type=int, default=8, help="files of one T_pad bucket per native call (1 = one file per call, the reference's loop)")
    p.add_argument("--resample", type=str, default="host", choices=["host", "device"],
                   help="where a file that is not at the model's rate is resampled.  host: `resample` on the CPU (the default).  device: the same "
                        "polyphase filter as a HIP kernel on the model's device (flowdec_amd.resample), summed in float64 and rounded once -- "
                        "the output files then differ from host mode by float32 rounding of the FIR.  A rate pair whose filter bank is over "
                        "the device resampler's cap falls back to the host path, with one printed line")
    p.add_argument("--gpus", type=int, default=1,
                   help="run the corpus on this many GPUs (cuda:0 .. cuda:N-1), one worker process each, batches spread by frame count; the "
                        "outputs, rtfs.csv and triples_list.txt are those of a one-process run (default 1: no child process)")
    p.add_argument("--eval", action="store_true",
                   help="pair lists only: after the run (after the merge of a --gpus N run), score the triples list just written with "
                        "flowdec_amd.eval_cli on one GPU -> metrics{suffix}.csv next to it; the files are scored as written to disk")
    p.add_argument("--eval-estoi", action="store_true", help="with --eval: also score ESTOI (eval_cli --estoi), a last column `estoi` of the CSV")
    p.add_argument("--eval-spectral", action="store_true",
                   help="with --eval: also score the multi-scale STFT and mel distances (eval_cli --spectral), two last columns `msstft` and `mel`")
    p.add_argument("--eval-align", type=float, default=None, metavar="MS",
                   help="with --eval: align every triple in time within +-MS milliseconds before scoring (eval_cli --align MS), two last columns "
                        "`lag_x_hat` and `lag_y`")
    p.add_argument("--eval-align-frac", action="store_true",
                   help="with --eval-align MS: sub-sample delays (eval_cli --align-frac); `lag_x_hat` and `lag_y` then hold fractions of a sample")
    p.add_argument("--eval-align-polarity", action="store_true",
                   help="with --eval-align MS: undo an inverted polarity before scoring (eval_cli --align-polarity), two further last columns "
                        "`pol_x_hat` and `pol_y`")
    p.add_argument("--eval-loudness", action="store_true",
                   help="with --eval: also measure the integrated loudness of x_hat, x and y (eval_cli --loudness), three columns `lufs_x_hat`, "
                        "`lufs_x`, `lufs_y` behind the metrics")
    p.add_argument("--eval-match-loudness", action="store_true",
                   help="with --eval: scale x_hat and y to the loudness of x before every metric (eval_cli --match-loudness; implies "
                        "--eval-loudness)")
    p.add_argument("--eval-ssnr", action="store_true",
                   help="with --eval: also score the segmental SNRs (eval_cli --ssnr), two columns `fwSSNR` and `SSNR` behind the other metrics")
    p.add_argument("--eval-loudness-range", action="store_true",
                   help="with --eval: also measure the loudness range of x_hat, x and y (eval_cli --loudness-range), three columns `lra_*`")
    p.add_argument("--eval-true-peak", action="store_true",
                   help="with --eval: also measure the true peak of x_hat, x and y (eval_cli --true-peak), three columns `dbtp_*`")
    p.add_argument("--target-lufs", type=target_lufs_arg, default=None, metavar="VALUE|input",
                   help="bring every written file to VALUE LUFS (integrated loudness, ITU-R BS.1770-4 / EBU R 128; R 128 asks for -23, the codec "
                        "package this project restates for -16), or with `input` to the integrated loudness of its own input file: ONE gain per "
                        "file, measured on the finished output, applied before it is written and outside the region --rtf times; "
                        "`loudness{suffix}.csv` (name, lufs, dbtp, gain_db, limited) records every file (default: off, the files are written "
                        "as the model gives them)")
    p.add_argument("--peak-ceiling", type=float, default=None, metavar="DBTP",
                   help="cap the gain of --target-lufs so that no written file's true peak (BS.1770-4 Annex 2) exceeds DBTP (a gain cap, not a "
                        "limiter; default -1.0 with --target-lufs, as R 128 asks).  Given alone: files over the ceiling are turned down to it, "
                        "the others are left as they are")
    p.add_argument("--share-gpu", action="store_true", help="with --gpus N: all N <= %d workers on cuda:0 (a test aid for one-GPU boxes)" % SHARE_GPU_MAX_RANKS)
    p.add_argument("--worker-rank", type=int, default=None, help=argparse.SUPPRESS)        # set by the launcher of a --gpus N run
    p.add_argument("--worker-world", type=int, default=None, help=argparse.SUPPRESS)
    p.add_argument("--worker-manifest", type=str, default=None, help=argparse.SUPPRESS)
    return p


def collect_files(files: str, single_file: bool) -> Tuple[List[str], Optional[List[str]]]:
    """-> (noisy paths, clean paths or None)."""
    if os.path.isfile(files):
        if single_file:
            return [files], None
        fl = read_list(files)
        return fl.inputs, fl.clean
    return sorted(glob.glob(f"{files}/*.wav")), None


@dataclass
class RunResult:
    """What a CLI run did: files enhanced, files skipped because they exceed the length limit of the chosen precision (but not
    --max-seconds) or because their workspace does not fit in device memory, files skipped as longer than --max-seconds."""
    n_done: int = 0
    n_over_precision_limit: int = 0
    n_too_long: int = 0
    gpu_seconds: float = 0.0      # --rtf: GPU time and audio duration over the files enhanced in this run
    audio_seconds: float = 0.0

    @property
    def exit_code(self) -> int:
        return 3 if self.n_over_precision_limit else 0


@dataclass
class FileJob:
    """One entry of the work list: where the input is, where the output goes, the clean reference of a pair list, and whether there
    is anything to compute (`pending` is False when the output exists and --skip-existing holds)."""
    index: int
    src: str
    dst: str
    clean: Optional[str]
    pending: bool


def plan_jobs(noisy: List[str], clean: Optional[List[str]], outdir: str, i_min: Optional[int], i_max: Optional[int],
              skip_existing: bool, exclude: Optional[str] = None):
    """The work list of a run as a generator of FileJob: the exclusion pattern first (it renumbers the list), then the inclusive
    index window [i_min, i_max] over what is left, then the exists-check."""
    entries = [(n, clean[k] if clean is not None else None) for k, n in enumerate(noisy) if exclude is None or exclude not in n]
    lo = 0 if i_min is None else max(i_min, 0)
    hi = len(entries) - 1 if i_max is None else min(i_max, len(entries) - 1)
    for index in range(lo, hi + 1):
        src, cl = entries[index]
        dst = os.path.join(outdir, os.path.basename(src))
        yield FileJob(index, src, dst, cl, pending=not (skip_existing and os.path.exists(dst)))


class GpuTimer:
    """`with GpuTimer(enabled) as t: ...` -> t.seconds = device time between entry and exit on the current stream (None when disabled)."""

    def __init__(self, enabled: bool):
        self.enabled, self.seconds = enabled, None

    def __enter__(self):
        if self.enabled:
            self._ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
            self._ev[0].record()
        return self

    def __exit__(self, *exc):
        if self.enabled and exc[0] is None:
            self._ev[1].record()
            torch.cuda.synchronize()
            self.seconds = self._ev[0].elapsed_time(self._ev[1]) / 1000.0
        return False


RTF_HEADER = "path,runtime,filetime,rtf"


def rtf_part_name(suffix: str, rank: int) -> str:
    return f"rtfs{suffix}.rank{rank}.csv"


LEVEL_HEADER = "name,lufs,dbtp,gain_db,limited"


def level_part_name(suffix: str, rank: int) -> str:
    return f"loudness{suffix}.rank{rank}.csv"


def result_part_name(suffix: str, rank: int) -> str:
    return f"result{suffix}.rank{rank}.json"


def manifest_name(suffix: str) -> str:
    return f"manifest{suffix}.json"


class RunLog:
    """The two side files of a run, in the reference's FORMATS (enhance.py:94,135,143): `rtfs{suffix}.csv` with the header
    path,runtime,filetime,rtf (--rtf) and `triples_list{suffix}.txt` with `clean ---> noisy ---> enhanced` lines (pair lists).
    The files are opened on __enter__ (a failing second open closes the first)."""

    def __init__(self, outdir: str, suffix: str, want_rtf: bool, want_triples: bool, part: Optional[int] = None, want_level: bool = False):
        """part = r: the log of worker r of a --gpus N run -- `rtfs{suffix}.rank{r}.csv` with the plan position (`self.position`, set by
        the caller before each batch) as an extra first column, and no triples list (the launcher writes that one).  want_level
        (--target-lufs / --peak-ceiling): also `loudness{suffix}.csv` (LEVEL_HEADER), as a part `loudness{suffix}.rank{r}.csv` with the
        position column for a worker."""
        self._paths = (os.path.join(outdir, f"rtfs{suffix}.csv" if part is None else rtf_part_name(suffix, part)) if want_rtf else None,
                       os.path.join(outdir, f"triples_list{suffix}.txt") if want_triples and part is None else None,
                       os.path.join(outdir, f"loudness{suffix}.csv" if part is None else level_part_name(suffix, part)) if want_level else None)
        self._stack = contextlib.ExitStack()
        self._rtf = self._tri = self._level = None
        self._part, self.position = part, 0
        self.runtime = self.filetime = 0.0

    def __enter__(self):
        with contextlib.ExitStack() as guard:
            self._rtf = guard.enter_context(open(self._paths[0], "w")) if self._paths[0] else None
            self._tri = guard.enter_context(open(self._paths[1], "w")) if self._paths[1] else None
            self._level = guard.enter_context(open(self._paths[2], "w")) if self._paths[2] else None
            self._stack = guard.pop_all()
        if self._rtf:
            print(RTF_HEADER if self._part is None else "position," + RTF_HEADER, file=self._rtf)
        if self._level:
            print(LEVEL_HEADER if self._part is None else "position," + LEVEL_HEADER, file=self._level)
        return self

    def level(self, dst: str, lufs: float, dbtp: float, gain_db: Optional[float], limited: bool):
        """One row of loudness{suffix}.csv: the file's name, its level as the model gave it, the gain applied (nan: none) and whether the
        ceiling capped it."""
        if self._level:
            row = [os.path.basename(dst), eval_cli.fmt(lufs), eval_cli.fmt(dbtp), eval_cli.fmt(float("nan") if gain_db is None else gain_db), str(int(limited))]
            print(("" if self._part is None else f"{self.position},") + ",".join(row), file=self._level)

    def __exit__(self, *exc):
        return self._stack.__exit__(*exc)

    def rtf(self, dst: str, runtime: float, filetime: float):
        print(runtime, filetime, "-> rtf =", runtime / filetime)
        self.runtime += runtime
        self.filetime += filetime
        if self._rtf:
            print(("" if self._part is None else f"{self.position},") + f"{dst},{runtime:.5f},{filetime:.5f},{runtime / filetime:.5f}", file=self._rtf)

    def triple(self, job: FileJob):
        if self._tri:
            print(f"{job.clean} ---> {job.src} ---> {job.dst}", file=self._tri)


def file_generator(model: FlowModel, seed: Optional[int], index: int):
    """The noise generator of file `index` of the work list: seeded SEED + index, so that a file's result does not depend on which
    files share its batch; None (the global device RNG, like the reference: model.py:512) without --seed."""
    return None if seed is None else torch.Generator(device=model.device).manual_seed(int(seed) + int(index))


def noise_kwargs(model: FlowModel, args, indices: List[int], batch: bool) -> dict:
    """The noise arguments of enhance (batch=False, one index) / enhance_batch for the files `indices` of the work list.  The regression
    model draws no noise: it takes none of them."""
    if isinstance(model, RegressionModel):
        return {}
    if args.rng == "native":
        seeds = [clip_seed(args.seed, i) for i in indices]
        return dict(seeds=seeds) if batch else dict(seed=seeds)
    gens = [file_generator(model, args.seed, i) for i in indices]
    return dict(generator=gens) if batch else dict(generator=gens[0])


def enhance_kwargs(model, args) -> dict:
    """The sampler / solver arguments of `enhance` and `enhance_batch` for the model's class: a FlowModel takes --N and --solver, a ScoreModel
    --N, --predictor, --corrector and --snr, a RegressionModel none (one network evaluation).  With --sampler ode a ScoreModel's are those of
    `enhance_ode_batch`: --N (the denoising step's dt = 1 / N), --ode-rtol, --ode-atol."""
    if ode_sampler(model, args):
        return dict(N=args.N, rtol=args.ode_rtol, atol=args.ode_atol)
    if isinstance(model, ScoreModel):
        return dict(N=args.N, predictor=args.predictor, corrector=args.corrector, snr=args.snr)
    if isinstance(model, RegressionModel):
        return {}
    if per_clip_control(args):
        return dict(N=args.N, solver=args.solver, step_control="clip")
    return dict(N=args.N, solver=args.solver)


def ode_sampler(model, args) -> bool:
    """--sampler ode on a score model: the files run through `ScoreModel.enhance_ode_batch`."""
    return isinstance(model, ScoreModel) and getattr(args, "sampler", "pc") == "ode"


def enhance_ode_files(model, clips, jobs: List[FileJob], args):
    """--sampler ode: the files `jobs` (waveforms `clips`, one T_pad bucket) as ONE `enhance_ode_batch` call, one step controller per file;
    prints every file's NFE (rtfs.csv has no column for it).  -> the enhanced waveforms."""
    outs, nfe = model.enhance_ode_batch(clips, return_nfe=True, **enhance_kwargs(model, args),
                                        **noise_kwargs(model, args, [job.index for job in jobs], batch=True))
    for job, n in zip(jobs, nfe):
        print(f"NFE {n}: {job.dst}")
    return outs


def per_clip_control(args) -> bool:
    """--step-control clip with an adaptive --solver: every file steps under its own controller (`FlowModel.enhance(step_control='clip')`)."""
    return getattr(args, "step_control", "batch") == "clip" and args.solver in ("dopri5", "tsit5")


def batchable(model, args) -> bool:
    """Whether the run can use ragged batches: the flow model's adaptive solvers step clip by clip unless --step-control clip gives
    every file its own controller; everything else runs in batches."""
    return not isinstance(model, FlowModel) or args.solver in ("euler", "midpoint", "heun2", "heun2_eulerlast") or per_clip_control(args)


def chunk_samples(model, args) -> Optional[int]:
    """--chunk-seconds -> the samples of one row at the model's rate (files with more take the long-form path), None when it is off."""
    if getattr(args, "chunk_seconds", None) is None:
        return None
    hop = model.feature_extractor._cfg()["hop"]
    return longform.row_samples(longform.chunk_row_frames(args.chunk_seconds, model.sampling_rate, hop), hop)


def resample_for_model(y: torch.Tensor, sr: int, model, mode: str = "host") -> torch.Tensor:
    """--resample: to the model's rate, on the host or on the model's device (`audio.resample_to`)."""
    return resample_to(y, sr, model.sampling_rate, mode, model.device)


def load_for_model(model: FlowModel, job: FileJob, res: RunResult, max_seconds: float, precision: str, length_limit: float = MAX_SECONDS,
                   long_samples: Optional[int] = None, resample_mode: str = "host"):
    """Load -> the reference's length rule (enhance.py:115,139; `length_limit` = --max-seconds) -> resample to the model rate
    (`resample_mode` = --resample).  -> waveform [C, L] or None (skipped).  A file of more than `long_samples` samples at the model's rate
    (--chunk-seconds) is exempt from the length rule: it runs in rows."""
    y, sr = load_wav(job.src)
    seconds = y.shape[-1] / sr
    if long_samples is not None and resampled_length(y.shape[-1], sr, model.sampling_rate) > long_samples:
        pass
    elif seconds > length_limit:
        res.n_too_long += 1
        print("Skipping file due to length:", job.src)
        return None
    elif seconds > max_seconds:
        res.n_over_precision_limit += 1
        print(f"Skipping file: {seconds:.1f} s exceeds the {max_seconds:g} s limit of precision={precision} "
              f"(the length limit is {length_limit:g} s; use --precision bf16 for files up to it):", job.src)
        return None
    if sr != model.sampling_rate:
        print("RESAMPLING from", sr, "to", model.sampling_rate)
        y = resample_for_model(y, sr, model, resample_mode)
    return y


def skip_over_memory(job: FileJob, res: RunResult, err: Exception) -> None:
    res.n_over_precision_limit += 1
    print(f"Skipping file: {err}:", job.src)


def level_wanted(args) -> bool:
    return getattr(args, "target_lufs", None) is not None or getattr(args, "peak_ceiling", None) is not None


def _file_level(w: torch.Tensor, sr: int, args, peak: bool = True):
    """(lufs, dbtp) of the FILE w [C, L] (or [L]): its channels' energies added and gated once, the largest true peak
    (loudness.file_level_batch, on the GPU, one staging).  peak=False: the loudness alone, dbtp NaN."""
    chans = list(w.detach().reshape(-1, w.shape[-1]).to(torch.float32))
    with torch.cuda.device(args.device):
        lufs, dbtp = loudness.file_level_batch([chans], sr, batch=max(len(chans), 1), device=args.device, peak=peak)
    return float(lufs[0]), float(dbtp[0])


def control_level(x_hat: torch.Tensor, y: torch.Tensor, job: FileJob, args, log: RunLog, sr: int) -> torch.Tensor:
    """--target-lufs / --peak-ceiling: the finished output x_hat of the input y (both at rate sr) -> what is written.  The level of the file
    is measured once (the channels of a file count as one programme), ONE gain follows from it (loudness.output_gain) and every sample gets
    ONE float32 multiply (loudness.normalize_loudness); a row goes to loudness{suffix}.csv.  A file with no finite level (under 400 ms,
    silent, a sample that is not finite) is written as it is, with a warning.  Without the switches: x_hat itself, nothing measured."""
    if not level_wanted(args):
        return x_hat
    lufs, dbtp = _file_level(x_hat, sr, args)
    ceiling = args.peak_ceiling
    if args.target_lufs is None:          # --peak-ceiling alone: 0 dB, capped
        gain, limited = loudness.output_gain(0.0, dbtp, 0.0, ceiling)
    else:
        ceiling = -1.0 if ceiling is None else ceiling
        target = _file_level(y, sr, args, peak=False)[0] if args.target_lufs == "input" else float(args.target_lufs)
        gain, limited = loudness.output_gain(lufs, dbtp, target, ceiling) if target == target and abs(target) != float("inf") else (None, False)
    log.level(job.dst, lufs, dbtp, gain, limited)
    if gain is None:
        print(f"warning: {job.dst}: lufs = {eval_cli.fmt(lufs)}, dbtp = {eval_cli.fmt(dbtp)}: no level to set (under 400 ms, silent or not finite); "
              f"the file is written as it is", file=sys.stderr)
        return x_hat
    return loudness.match_loudness(x_hat.to(torch.float32), 0.0, gain)


def enhance_file(model: FlowModel, job: FileJob, args, log: RunLog, res: RunResult, max_seconds: float, y=None) -> None:
    """One file per native call (the reference's loop): load -> enhance (timed under --rtf) -> save.  Updates `res`.  `y`: the file's
    waveform when the caller has already loaded (and resampled) it."""
    long_samples = chunk_samples(model, args)
    if y is None:
        y = load_for_model(model, job, res, max_seconds, args.precision, args.max_seconds, long_samples, resample_mode=getattr(args, "resample", "host"))
    if y is None:
        return
    sr = model.sampling_rate
    if long_samples is not None and y.shape[-1] > long_samples:   # --chunk-seconds: rows of one bucket, a workspace that does not grow with the file
        row_frames = longform.chunk_row_frames(args.chunk_seconds, sr, model.feature_extractor._cfg()["hop"])
        rows_per_call = max(args.batch_files, 1)
        print(f"Long file: {y.shape[-1] / sr:.1f} s in rows of {row_frames} frames, {rows_per_call} per call "
              f"(--chunk-seconds: exempt from --max-seconds and from the limit of precision={args.precision}):", job.src)
        try:
            with GpuTimer(args.rtf) as timer:
                x_hat = model.enhance_long(y, N=args.N, solver=args.solver, seed=[clip_seed(args.seed, job.index)], row_frames=row_frames,
                                           halo_frames=longform.chunk_halo_frames(row_frames), rows_per_call=rows_per_call)
        except WorkspaceTooLarge as err:   # rows_per_call rows of --chunk-seconds do not fit: the file is skipped, the run goes on
            skip_over_memory(job, res, err)
            return
        if timer.seconds is not None:
            log.rtf(job.dst, timer.seconds, y.shape[-1] / sr)
        save_wav(job.dst, control_level(x_hat, y, job, args, log, sr).cpu(), sr)
        res.n_done += 1
        return
    # use_graph=False: every file has its own length, and a replay would not be faster anyway -- a one-clip solve is bound by the GPU,
    # not by the host's launches (profiles/r02_graph_cost.txt: eager 18.06 ms, replay 18.10 ms; capture + instantiate 2.4 ms)
    try:
        with GpuTimer(args.rtf) as timer:
            if ode_sampler(model, args):   # a batch of one: the same per-file controller, so the file's waveform is its batched one
                x_hat = enhance_ode_files(model, [y], [job], args)[0]
            else:
                x_hat = model.enhance(y, use_graph=False, **enhance_kwargs(model, args), **noise_kwargs(model, args, [job.index], batch=False))
    except WorkspaceTooLarge as err:
        skip_over_memory(job, res, err)
        return
    if timer.seconds is not None:
        log.rtf(job.dst, timer.seconds, y.shape[-1] / sr)
    save_wav(job.dst, control_level(x_hat, y, job, args, log, sr).cpu(), sr)
    res.n_done += 1


def plan_batches(model: FlowModel, jobs: List[FileJob], batch_files: int, length_limit: float = MAX_SECONDS, long_samples: Optional[int] = None):
    """Buckets the pending jobs by the frame count their spectrogram pads to (from the wav HEADERS: nothing is decoded here) and cuts
    every bucket into batches of at most `batch_files` files, in work-list order.  Multi-channel files, unreadable headers and files
    the length rule will skip go through the one-file path (their own messages), and so do files of more than `long_samples` samples
    (--chunk-seconds: they run in rows).  -> list of lists of FileJob."""
    hop = model.feature_extractor._cfg()["hop"]
    bucketed, lengths, singles = [], [], []
    for job in jobs:
        try:
            n, sr, channels = wav_info(job.src)
        except Exception:   # an unreadable file fails in its own one-file call, with the reference's behaviour (an exception)
            singles.append([job]); continue
        if long_samples is not None and resampled_length(n, sr, model.sampling_rate) > long_samples:
            singles.append([job]); continue
        if channels != 1 or n / sr > length_limit or batch_files <= 1:
            singles.append([job]); continue
        bucketed.append(job); lengths.append(resampled_length(n, sr, model.sampling_rate))
    return [[bucketed[i] for i in idx] for _, idx in plan_clip_batches(lengths, hop, batch_files)] + singles


def enhance_batch_files(model: FlowModel, batch: List[FileJob], args, log: RunLog, res: RunResult, max_seconds: float) -> None:
    """One ragged native call for the files of `batch` (same T_pad bucket).  Every output equals the one-file call bit for bit."""
    loaded = [(job, load_for_model(model, job, res, max_seconds, args.precision, args.max_seconds, resample_mode=getattr(args, "resample", "host")))
              for job in batch]
    loaded = [(job, y) for job, y in loaded if y is not None]
    if not loaded:
        return
    sr = model.sampling_rate
    noise = noise_kwargs(model, args, [job.index for job, _ in loaded], batch=True)
    try:
        with GpuTimer(args.rtf) as timer:
            if ode_sampler(model, args):
                outs = enhance_ode_files(model, [y for _, y in loaded], [job for job, _ in loaded], args)
            else:
                outs = model.enhance_batch([y for _, y in loaded], **enhance_kwargs(model, args), **noise)
    except WorkspaceTooLarge:   # the batch does not fit: one call per file (each result is the same, bit for bit)
        for job, y in loaded:
            enhance_file(model, job, args, log, res, max_seconds, y=y)
        return
    total = sum(y.shape[-1] for _, y in loaded) / sr
    for (job, y), x_hat in zip(loaded, outs):
        if timer.seconds is not None:   # the batch's time, split in proportion to the files' durations
            log.rtf(job.dst, timer.seconds * (y.shape[-1] / sr) / total, y.shape[-1] / sr)
        save_wav(job.dst, control_level(x_hat, y, job, args, log, sr).cpu(), sr)
        res.n_done += 1


# ------------------------------------------------------------------------------------------------
# --gpus N: manifest, cost model, launcher, merge
# ------------------------------------------------------------------------------------------------
class WorkerFailed(RuntimeError):
    """A worker of a --gpus N run did not finish; the message names the rank and shows its last lines."""


def write_manifest(path: str, jobs: List[FileJob]) -> None:
    """The work list of a --gpus N run, planned ONCE by the launcher: the workers read it and do not repeat the exists-check."""
    with open(path, "w") as f:
        json.dump({"jobs": [dict(index=j.index, src=j.src, dst=j.dst, clean=j.clean, pending=j.pending) for j in jobs]}, f)


def read_manifest(path: str) -> List[FileJob]:
    with open(path, "r") as f:
        return [FileJob(int(j["index"]), j["src"], j["dst"], j["clean"], bool(j["pending"])) for j in json.load(f)["jobs"]]


def batch_cost(model, batch: List[FileJob], args) -> int:
    """The cost of one batch of the plan in padded STFT frames, from the wav headers: a bucketed batch costs files x T_pad, a single file
    channels x padded frames, a --chunk-seconds file channels x rows x row frames (`longform.plan_rows`); an unreadable header costs 0 (the
    file fails in its own call), and so does a file the length rule will skip.  A heuristic -- GPU time taken as proportional to the frames
    in flight, whatever the batch size and the bucket; how evenly it spreads a real corpus over the ranks has not been measured."""
    hop = model.feature_extractor._cfg()["hop"]
    long_samples = chunk_samples(model, args)
    try:
        n, sr, channels = wav_info(batch[0].src)
    except Exception:
        return 0
    n = resampled_length(n, sr, model.sampling_rate)
    if len(batch) > 1:
        return len(batch) * padded_frames_of(n, hop)
    if long_samples is not None and n > long_samples:
        row_frames = longform.chunk_row_frames(args.chunk_seconds, model.sampling_rate, hop)
        return channels * len(longform.plan_rows(n, hop, row_frames, longform.chunk_halo_frames(row_frames))) * row_frames
    if n / model.sampling_rate > args.max_seconds:
        return 0
    return channels * padded_frames_of(n, hop)


def visible_gpus() -> int:
    """torch.cuda.device_count() of a short-lived child process: the launcher itself never opens the GPU."""
    r = subprocess.run([sys.executable, "-c", "import torch; print(torch.cuda.device_count())"], capture_output=True, text=True, timeout=300)
    try:
        return int(r.stdout.strip().splitlines()[-1])
    except (IndexError, ValueError):
        raise RuntimeError("could not read the number of visible GPUs: " + (r.stdout + r.stderr)[-500:])


def merge_parts(outdir: str, suffix: str, world: int, jobs: List[FileJob], want_rtf: bool, want_triples: bool, want_level: bool = False) -> RunResult:
    """The launcher's last step: the workers' `rtfs{suffix}.rank{r}.csv` rows sorted by plan position (rows of one position keep their
    order; the position column is dropped) -> `rtfs{suffix}.csv`, the rows and order of a one-process run; `triples_list{suffix}.txt` from
    the work list; the workers' RunResults summed.  want_level: `loudness{suffix}.csv` from the `loudness{suffix}.rank{r}.csv` parts in
    the same way.  Removes the part files it read."""
    res, rows, used, level_rows = RunResult(), [], [], []
    for r in range(world):
        path = os.path.join(outdir, result_part_name(suffix, r))
        with open(path, "r") as f:
            part = json.load(f)
        used.append(path)
        res.n_done += int(part["n_done"]); res.n_over_precision_limit += int(part["n_over_precision_limit"]); res.n_too_long += int(part["n_too_long"])
        res.gpu_seconds += float(part["gpu_seconds"]); res.audio_seconds += float(part["audio_seconds"])
        if want_rtf:
            path = os.path.join(outdir, rtf_part_name(suffix, r))
            with open(path, "r") as f:
                lines = f.read().splitlines()
            used.append(path)
            for k, line in enumerate(lines[1:]):
                if line.strip():
                    pos, row = line.split(",", 1)
                    rows.append((int(pos), r, k, row))
        if want_level:
            path = os.path.join(outdir, level_part_name(suffix, r))
            with open(path, "r") as f:
                lines = f.read().splitlines()
            used.append(path)
            level_rows += [(int(line.split(",", 1)[0]), r, k, line.split(",", 1)[1]) for k, line in enumerate(lines[1:]) if line.strip()]
    if want_level:
        with open(os.path.join(outdir, f"loudness{suffix}.csv"), "w") as f:
            print(LEVEL_HEADER, file=f)
            for _, _, _, row in sorted(level_rows):
                print(row, file=f)
    if want_rtf:
        with open(os.path.join(outdir, f"rtfs{suffix}.csv"), "w") as f:
            print(RTF_HEADER, file=f)
            for _, _, _, row in sorted(rows):
                print(row, file=f)
    if want_triples:
        with open(os.path.join(outdir, f"triples_list{suffix}.txt"), "w") as f:
            for job in jobs:
                print(f"{job.clean} ---> {job.src} ---> {job.dst}", file=f)
    for path in used:
        os.remove(path)
    return res


FATAL_STATUS = (134, 139)   # abort / segmentation fault as a shell reports them; a negative status is the signal itself


def launch_workers(argv: List[str], world: int, manifest: str, share_gpu: bool):
    """Starts the `world` workers at once (fresh processes of this module, the environment untouched), relays their output line by line
    prefixed `[rank r]` and waits for all of them.  -> [(exit status, last lines)].  A worker that ends by a signal, an abort or a
    segmentation fault ends the run: the others are terminated and WorkerFailed is raised."""
    procs, tails, threads = [], [], []
    lock = threading.Lock()

    def relay(r, pipe, tail):
        for line in pipe:
            tail.append(line.rstrip("\n"))
            with lock:
                print(f"[rank {r}] {line}", end="", flush=True)

    try:
        for r in range(world):
            cmd = [sys.executable, "-m", "flowdec_amd.enhance_cli"] + list(argv) + ["--worker-rank", str(r), "--worker-world", str(world),
                                                                                    "--worker-manifest", manifest]
            procs.append(subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, bufsize=1))
            tails.append(collections.deque(maxlen=20))
            threads.append(threading.Thread(target=relay, args=(r, procs[-1].stdout, tails[-1]), daemon=True))
            threads[-1].start()
        pending = set(range(world))
        while pending:
            for r in sorted(pending):
                rc = procs[r].poll()
                if rc is None:
                    continue
                pending.discard(r)
                if rc < 0 or rc in FATAL_STATUS:
                    threads[r].join(timeout=5)
                    raise WorkerFailed(f"rank {r} ended with status {rc} (signal, abort or segmentation fault): the other workers were stopped, "
                                       f"nothing more is started on a GPU that may have faulted; the part files stay in --outdir.  Its last lines:\n"
                                       + "\n".join(tails[r]))
            if pending:
                time.sleep(0.05)
    finally:
        for p in procs:
            if p.poll() is None:
                p.terminate()
        for p in procs:
            try:
                p.wait(timeout=30)
            except subprocess.TimeoutExpired:
                p.kill(); p.wait()
        for t in threads:
            t.join(timeout=5)
    return [(p.returncode, list(t)) for p, t in zip(procs, tails)]


def evaluate_triples(args, suffix: str) -> None:
    """--eval: SI-SxR and LogSpecMSE (--eval-estoi: and ESTOI; --eval-spectral: and msstft, mel; --eval-align MS: aligned in time first) of
    `triples_list{suffix}.txt` -> `metrics{suffix}.csv` beside it (flowdec_amd/eval_cli.py)."""
    with torch.cuda.device(args.device):
        eval_cli.run(["--triples", os.path.join(args.outdir, f"triples_list{suffix}.txt"), "--out", os.path.join(args.outdir, f"metrics{suffix}.csv"),
                      "--batch-files", str(max(args.batch_files, 1))] + (["--estoi"] if getattr(args, "eval_estoi", False) else [])
                     + (["--spectral"] if getattr(args, "eval_spectral", False) else [])
                     + (["--align", repr(float(args.eval_align))] if getattr(args, "eval_align", None) is not None else [])
                     + (["--align-frac"] if getattr(args, "eval_align_frac", False) else [])
                     + (["--align-polarity"] if getattr(args, "eval_align_polarity", False) else [])
                     + (["--loudness"] if getattr(args, "eval_loudness", False) else [])
                     + (["--match-loudness"] if getattr(args, "eval_match_loudness", False) else [])
                     + (["--loudness-range"] if getattr(args, "eval_loudness_range", False) else [])
                     + (["--true-peak"] if getattr(args, "eval_true_peak", False) else [])
                     + (["--ssnr"] if getattr(args, "eval_ssnr", False) else []))


def run_launcher(args, parser, argv: List[str]) -> RunResult:
    """The launching process of a --gpus N run (module docstring).  It loads no checkpoint and opens no GPU, except for --eval after the
    merge."""
    suffix = f"_{args.i_min}-{args.i_max}" if args.i_max else ""
    if not args.share_gpu:
        have = visible_gpus()
        if args.gpus > have:
            parser.error(f"--gpus {args.gpus} asks for more GPUs than the {have} visible on this node (no worker was started; --share-gpu puts "
                         f"several workers on one GPU, for tests)")
    noisy, clean = collect_files(args.files, args.single_file)
    jobs = list(plan_jobs(noisy, clean, args.outdir, args.i_min, args.i_max, args.skip_existing, args.exclude_files_matching))
    manifest = os.path.join(args.outdir, manifest_name(suffix))
    for stale in glob.glob(os.path.join(glob.escape(args.outdir), f"*{suffix}.rank*.*")):      # parts a failed earlier run left for diagnosis
        if re.fullmatch(r"(rtfs|result|loudness)%s\.rank\d+\.(csv|json)" % re.escape(suffix), os.path.basename(stale)):
            os.remove(stale)
    write_manifest(manifest, jobs)
    worker_argv = list(argv) + (["--seed", str(args.seed)] if args.seed is not None else [])
    t0 = time.perf_counter()
    ended = launch_workers(worker_argv, args.gpus, manifest, args.share_gpu)
    wall = time.perf_counter() - t0
    failed = [(r, rc, tail) for r, (rc, tail) in enumerate(ended)
              if rc not in (0, 3) or not os.path.exists(os.path.join(args.outdir, result_part_name(suffix, r)))]
    if failed:
        raise WorkerFailed("\n".join(f"rank {r} ended with status {rc}; its last lines:\n" + "\n".join(tail) for r, rc, tail in failed)
                           + f"\n{len(failed)} of {args.gpus} workers failed; the others finished.  The part files stay in {args.outdir}; a rerun with "
                             f"--skip-existing completes what is missing.")
    res = merge_parts(args.outdir, suffix, args.gpus, jobs, want_rtf=args.rtf, want_triples=clean is not None, want_level=level_wanted(args))
    os.remove(manifest)
    if args.rtf and res.gpu_seconds > 0:
        print(f"total: {res.audio_seconds:.2f} s of audio in {res.gpu_seconds:.3f} s of GPU time -> rtf = {res.gpu_seconds / res.audio_seconds:.5f} "
              f"({res.audio_seconds / res.gpu_seconds:.1f} x real time)")
        print(f"{args.gpus} workers: {res.audio_seconds:.2f} s of audio in {wall:.3f} s of wall clock, start-up and checkpoint loading included "
              f"({res.audio_seconds / wall:.1f} x real time)")
    else:
        print(f"{args.gpus} workers: {res.n_done} files in {wall:.3f} s of wall clock, start-up and checkpoint loading included")
    if args.eval and clean is not None:
        evaluate_triples(args, suffix)
    return res


def main(argv=None, model: Optional[FlowModel] = None) -> int:
    """Runs the CLI and returns the number of files enhanced (the detailed result: `run()`)."""
    return run(argv, model).n_done


def cli(argv=None) -> int:
    """Console entry point: exit status 0, or 3 when files were skipped only because of the chosen precision's length limit; 1 when a
    worker of a --gpus N run failed."""
    try:
        return run(argv).exit_code
    except WorkerFailed as err:
        print(f"flowdec_amd: {err}", file=sys.stderr)
        return 1


def run(argv=None, model: Optional[FlowModel] = None) -> RunResult:
    parser = build_parser()
    argv = list(sys.argv[1:] if argv is None else argv)
    args = parser.parse_args(argv)
    if args.chunk_seconds is not None:
        if not args.chunk_seconds > 0:
            parser.error("--chunk-seconds must be positive")
        if args.rng != "native":
            parser.error("--chunk-seconds needs --rng native: the rows of a file share the library's noise by absolute frame")
        if args.model not in ("auto", "flow"):
            parser.error("--chunk-seconds needs a flow model (got --model %s)" % args.model)
        if args.solver not in ("euler", "midpoint", "heun2", "heun2_eulerlast"):
            parser.error("--chunk-seconds needs a fixed-step --solver (euler, midpoint, heun2, heun2_eulerlast)")
    if (args.eval_align_frac or args.eval_align_polarity) and args.eval_align is None:
        parser.error("--eval-align-frac and --eval-align-polarity need --eval-align MS")
    worker = args.worker_rank is not None
    if args.gpus < 1:
        parser.error("--gpus must be at least 1")
    if worker:
        if args.worker_world is None or args.worker_manifest is None or not 0 <= args.worker_rank < args.worker_world:
            parser.error("a worker needs its rank, the world size and the manifest (they are set by the launcher of a --gpus N run)")
        args.device = "cuda:0" if args.share_gpu else f"cuda:{args.worker_rank}"
    elif args.gpus > 1:
        if args.device != "cuda:0":
            parser.error(f"--gpus {args.gpus} places worker r on cuda:r: it does not combine with --device {args.device}")
        if args.share_gpu and args.gpus > SHARE_GPU_MAX_RANKS:
            parser.error(f"--share-gpu takes at most {SHARE_GPU_MAX_RANKS} workers (got --gpus {args.gpus})")
        if model is not None:
            raise ValueError(f"run(model=...) with --gpus {args.gpus}: the workers are fresh processes and load --ckpt themselves")
    os.makedirs(args.outdir, exist_ok=True)
    if args.rng == "native" and args.seed is None:
        args.seed = int.from_bytes(os.urandom(8), "little")
        print(f"flowdec_amd: --rng native without --seed: using --seed {args.seed}")
    if args.gpus > 1 and not worker:
        return run_launcher(args, parser, argv)
    if model is None:
        print("Loading model from checkpoint...")
        model = load_from_checkpoint(args.ckpt, map_location=args.device, ema=args.ema, precision=args.precision, model=args.model)
        print("Done loading model.")
    if args.chunk_seconds is not None and not isinstance(model, FlowModel):
        parser.error("--chunk-seconds needs a flow checkpoint (this one is a %s)" % type(model).__name__)
    if args.sampler == "ode":
        if not isinstance(model, ScoreModel):
            parser.error("--sampler ode needs a score model (this one is a %s)" % type(model).__name__)
        if not args.ode_atol > 0 or not args.ode_rtol >= 0:
            parser.error("--sampler ode needs --ode-atol > 0 and --ode-rtol >= 0")
        print("flowdec_amd: --sampler ode: --predictor, --corrector and --snr are ignored")
    max_seconds = min(args.max_seconds, PRECISION_MAX_SECONDS.get(args.precision, args.max_seconds))
    settings = ", ".join(f"{k}={v}" for k, v in enhance_kwargs(model, args).items()) or "one network evaluation"
    print(f"flowdec_amd: model={type(model).__name__}, precision={args.precision} ({PRECISION_NOTE[args.precision]}), {settings}, "
          f"files per native call <= {max(args.batch_files, 1)}")
    res = RunResult()
    suffix = f"_{args.i_min}-{args.i_max}" if args.i_max else ""
    if worker:
        jobs, clean = read_manifest(args.worker_manifest), None
    else:
        noisy, clean = collect_files(args.files, args.single_file)
        jobs = list(plan_jobs(noisy, clean, args.outdir, args.i_min, args.i_max, args.skip_existing, args.exclude_files_matching))
    plan = plan_batches(model, [j for j in jobs if j.pending], args.batch_files if batchable(model, args) else 1, args.max_seconds,
                        chunk_samples(model, args))
    mine = range(len(plan))
    if worker:      # the plan is the one-process plan; this rank runs its share of it, in plan order
        mine = balance([batch_cost(model, batch, args) for batch in plan], args.worker_world)[args.worker_rank]
        print(f"flowdec_amd: worker {args.worker_rank} of {args.worker_world} on {args.device}: {len(mine)} of {len(plan)} batches")
    if level_wanted(args):
        try:
            loudness.check_rate(model.sampling_rate)
        except ValueError as err:
            parser.error(f"--target-lufs / --peak-ceiling: {err}")
    with RunLog(args.outdir, suffix, want_rtf=args.rtf, want_triples=clean is not None, part=args.worker_rank, want_level=level_wanted(args)) as log:
        for position in mine:
            batch = plan[position]
            log.position = position
            if len(batch) == 1:
                enhance_file(model, batch[0], args, log, res, max_seconds)
            else:
                enhance_batch_files(model, batch, args, log, res, max_seconds)
        for job in jobs:      # the pair list names every file of the window, enhanced now or found existing (enhance.py:143)
            log.triple(job)
        if args.rtf and log.runtime > 0:
            print(f"total: {log.filetime:.2f} s of audio in {log.runtime:.3f} s of GPU time -> rtf = {log.runtime / log.filetime:.5f} "
                  f"({log.filetime / log.runtime:.1f} x real time)")
    res.gpu_seconds, res.audio_seconds = log.runtime, log.filetime
    if worker:
        with open(os.path.join(args.outdir, result_part_name(suffix, args.worker_rank)), "w") as f:
            json.dump(dict(n_done=res.n_done, n_over_precision_limit=res.n_over_precision_limit, n_too_long=res.n_too_long,
                           gpu_seconds=res.gpu_seconds, audio_seconds=res.audio_seconds), f)
    elif args.eval and clean is not None:
        evaluate_triples(args, suffix)
    return res


if __name__ == "__main__":
    sys.exit(cli())
