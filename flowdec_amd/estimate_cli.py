"""Estimates beta and sigma_y from a list of (clean, coded) pairs on the GPU: the reference's scripts/estimate_flowdec_params.py.

    python -m flowdec_amd.estimate_cli --pairs-file pairs.txt --alpha 0.3 --nfft 1534 --hop 384 [--per-band] [--n-samples 2500]
                                       [--seed 302] [--qx 0.997] [--qrmse 0.997] [--outfile-suffix S] [--overwrite] [--compare-ckpt CKPT]
                                       [--align MS [--align-frac] [--align-polarity]]

Input: lines `clean ---> coded` (--delim).  --n-samples of them are drawn without replacement and each pair is cropped at a random
position (or zero-padded) to --sample-duration seconds, with the script's own sequence of NumPy draws (flowdec_amd/estimate.py:
select_pairs, crop_or_pad_pair).  Every file is loaded like eval_cli's: mean of the channels, resampled to --sr with
lowpass_filter_width=256 when its rate differs.

Output, named and formatted as the script's: `flowdec_autoparams_nfft{nfft}_hop{hop}_alpha{alpha}_seed{seed}[_n{N}][_perband][_{suffix}].txt`
beside the pairs file, with the `=== Results ===` lines that are also printed; with --per-band the curve sigma_y[f] goes to the same name
with `.txt` replaced by `sigy_perband.npy` (so it ends in `_perbandsigy_perband.npy`, as the script's does).  If the text file exists
and --overwrite is not given, its contents are printed and nothing is computed.

--compare-ckpt CKPT then prints the checkpoint's beta and sigma_y beside the estimates (see `compare_with_ckpt`).

--align MS [--align-frac] [--align-polarity] [--align-q 64] [--align-taps 32] (off by default; without --align nothing changes) is for
pairs from a codec that is not this chain's own and brings a delay -- a whole number of samples, a fraction of one where a resampler sits
in its path -- or an inverted polarity: a delay of tau samples puts 2 sin(omega tau / 2) of every component's own magnitude into the
difference the sigma_y curve measures.  Right after loading and before the crop / pad rule, every coded file is aligned against its clean
file within +-MS milliseconds and both are cut to their common support, on the GPU in batches of --batch-pairs (flowdec_amd/align.py:
align_pairs; eval_cli's --align switches with the same meaning).  What is printed on stdout and the results file keep their text (the Args
line names the new switches); one alignment summary line (the smallest and the largest lag, the count of non-zero lags and of inverted
pairs) and the warnings for a lag at the edge of the search and an empty support go to stderr."""
import argparse
import contextlib
import os
import sys
import tempfile
from typing import List, Optional

import numpy as np
import torch

from . import align
from . import estimate as E
from .audio import RESAMPLE_HELP, load_mono
from .checkpoint import _cfg_get, _to_plain
from .model import sigma_y_from_file


def rreplace(s: str, old: str, new: str, occurrence: int = 1) -> str:
    return new.join(s.rsplit(old, occurrence))


def outfile_paths(args):
    """-> (text file, per-band curve file): the script's naming rule (:120-127, :169)."""
    suffix = f"_n{args.n_samples}" if args.n_samples != 2500 else ""
    suffix += "_perband" if args.per_band else ""
    suffix += f"_{args.outfile_suffix}" if args.outfile_suffix is not None else ""
    txt = os.path.join(os.path.dirname(args.pairs_file), f"flowdec_autoparams_nfft{args.nfft}_hop{args.hop}_alpha{args.alpha}_seed{args.seed}{suffix}.txt")
    return txt, rreplace(txt, ".txt", "sigy_perband.npy")


def result_lines(args, res: E.EstimateResult, curve_path: Optional[str]) -> List[str]:
    """The lines under `=== Results ===` (:185-191), with the script's formats."""
    lines = [f"   \tq{args.qx}( |x|  ) = {res.abs_quantile_x:.3f}, max( |x|  ) = {res.max_abs_x:.3f}"]
    if args.per_band:
        lines.append(f"-->\tbeta={res.beta:.2f}, sigma_y=<written to {curve_path}>")
    else:
        lines.append(f"   \tq{args.qrmse}( RMSE ) = {res.rmse_quantile:.3f}, max( RMSE ) = {res.rmse_max:.3f}")
        lines.append(f"-->\tbeta={res.beta:.2f}, sigma_y={res.sigma_y:.2f}")
    return lines


# ---- --compare-ckpt ----------------------------------------------------------------------------------------------------------------------
def ckpt_params(ckpt: dict):
    """-> (beta, sigma_y, kernel_bandwidth, factor) of a loaded checkpoint object: beta from hyper_parameters.model.feature_extractor
    (0.33 where absent, as checkpoint.model_from_checkpoint builds it), sigma_y from the state dict (a float, or float64 [F] for a curve; None where the
    checkpoint has none), and the smoothing its config applied to the curve file (hyper_parameters.model.sigma_y; the presets' 3 and 1)."""
    hp = _to_plain(ckpt["hyper_parameters"]) if ckpt.get("hyper_parameters") is not None else None
    mcfg = _cfg_get(hp, "model") or {}
    beta = float((mcfg.get("feature_extractor") or {}).get("beta", 0.33))
    sd = ckpt.get("_pl_ema_state_dict") or ckpt.get("state_dict") or ckpt
    sig = sd.get("sigma_y") if hasattr(sd, "get") else None
    if sig is not None:
        sig = np.asarray(torch.as_tensor(sig).detach().cpu().double().reshape(-1).numpy())
        sig = float(sig[0]) if sig.size == 1 else sig
    scfg = mcfg.get("sigma_y") if isinstance(mcfg.get("sigma_y"), dict) else {}
    return beta, sig, float(scfg.get("kernel_bandwidth", 3)), float(scfg.get("factor", 1))


def smoothed(curve: np.ndarray, kernel_bandwidth: float, factor: float) -> np.ndarray:
    """The curve as a model built from its file would hold it: model.sigma_y_from_file on a temporary copy."""
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "curve.npy")
        np.save(path, np.asarray(curve))
        return sigma_y_from_file(path, factor=factor, kernel_bandwidth=kernel_bandwidth).reshape(-1).numpy()


def compare_with_ckpt(res: E.EstimateResult, ckpt: dict) -> List[str]:
    """Lines that set the checkpoint's beta and sigma_y beside the estimates.  Two curves: the relative L2 distance
    |ckpt - smoothed(estimate)| / |ckpt|, the estimate smoothed as sigma_y_from_file smooths a curve file.  A curve against a scalar: the
    curve's mean beside the scalar."""
    beta, sig, bw, factor = ckpt_params(ckpt)
    lines = ["=== Checkpoint ===", f"   \tbeta: checkpoint {beta:.4f}, estimate {res.beta:.4f} (estimate / checkpoint = {res.beta / beta:.3f})"]
    est = res.sigma_y
    if sig is None:
        lines.append("   \tsigma_y: the checkpoint holds none")
    elif np.ndim(sig) == 0 and np.ndim(est) == 0:
        lines.append(f"   \tsigma_y: checkpoint {sig:.4f}, estimate {est:.4f} (estimate / checkpoint = {est / sig:.3f})")
    elif np.ndim(sig) == 1 and np.ndim(est) == 1:
        if len(sig) != len(est):
            lines.append(f"   \tsigma_y: checkpoint curve of {len(sig)} bands, estimate of {len(est)}: not comparable")
        else:
            sm = smoothed(est, bw, factor)
            rel = float(np.linalg.norm(sig - sm) / np.linalg.norm(sig))
            lines.append(f"   \tsigma_y: curves of {len(sig)} bands, mean checkpoint {sig.mean():.4f}, mean estimate {sm.mean():.4f} (smoothed, bandwidth "
                         f"{bw:g}), relative L2 distance {rel:.4f}")
    else:
        a, b = (float(np.mean(sig)), float(np.mean(est)))
        lines.append(f"   \tsigma_y: checkpoint {'curve, mean' if np.ndim(sig) else 'scalar'} {a:.4f}, estimate {'curve, mean' if np.ndim(est) else 'scalar'} "
                     f"{b:.4f} (run {'with' if np.ndim(sig) else 'without'} --per-band to compare like with like)")
    return lines


# ---- the run -----------------------------------------------------------------------------------------------------------------------------
def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="Estimate a FlowDec model's beta and sigma_y from (clean, coded) pairs on MI355X")
    p.add_argument("--pairs-file", type=str, required=True)
    p.add_argument("--delim", type=str, default=" ---> ")
    p.add_argument("--alpha", type=float, required=True, help="Amplitude compression exponent")
    p.add_argument("--nfft", type=int, required=True)
    p.add_argument("--hop", type=int, required=True)
    p.add_argument("--sr", type=int, default=48000, help="the rate every file is brought to; with --sample-duration it sets the crop length "
                   "(the reference ignores both and crops to 96000 samples: the same at the defaults)")
    p.add_argument("--n-samples", type=int, default=2500)
    p.add_argument("--sample-duration", type=float, default=2.0, help="seconds every pair is cropped or padded to (see --sr)")
    p.add_argument("--seed", type=int, default=302)
    p.add_argument("--qx", type=float, default=0.997,
                   help="Quantile of the global distribution of clean audio x that we will rescale to 1.0 (via *beta). 0.997 by default.")
    p.add_argument("--qrmse", type=float, default=0.997,
                   help="Quantile of the RMSEs of clean x vs coded y that can be used as a reasonable default sigma_y. 0.997 by default.")
    p.add_argument("--per-band", action="store_true", help="frequency-dependent sigma_y: --qrmse is then taken for each band separately")
    p.add_argument("--outfile-suffix", type=str, required=False, help="Suffix to append to the results filename")
    p.add_argument("--overwrite", action="store_true", help="recalculate and overwrite the results file even if it exists")
    p.add_argument("--device", type=int, default=0, help="Index of the GPU to use")
    p.add_argument("--batch-pairs", type=int, default=64, help="pairs per native call")
    p.add_argument("--compare-ckpt", type=str, default=None, help="a checkpoint whose beta and sigma_y are printed beside the estimates")
    p.add_argument("--resample", type=str, default="host", choices=["host", "device"], help=RESAMPLE_HELP)
    align.add_pair_arguments(p)
    return p


def run(argv=None, out=None) -> Optional[E.EstimateResult]:
    """-> the estimate, or None where an existing results file was printed instead."""
    out = out or sys.stdout
    parser = build_parser()
    args = parser.parse_args(list(sys.argv[1:] if argv is None else argv))
    aligner = None
    if args.align is not None or args.align_frac or args.align_polarity:
        try:
            aligner = align.PairAligner(args, args.sr, args.batch_pairs, device=args.device)
        except ValueError as err:
            parser.error(str(err))
    else:                       # the Args line of a run without alignment keeps its text
        for name in ("align", "align_frac", "align_polarity", "align_q", "align_taps"):
            delattr(args, name)
    print(args, file=sys.stderr)
    txt, curve_path = outfile_paths(args)
    if os.path.isfile(txt) and not args.overwrite:
        print("Output file exists, printing its contents:", file=sys.stderr)
        with open(txt, "r") as f:
            for line in f:
                print(line.rstrip("\n"), file=out)
        return None
    print("Running...", file=sys.stderr)
    with open(args.pairs_file, "r") as f:
        lines = [l.strip() for l in f.readlines()]
    _, pairs = E.select_pairs(lines, args.n_samples, args.seed, args.delim)
    target = int(args.sample_duration * args.sr)
    xs, ys = [], []
    with (torch.cuda.device(args.device) if args.resample == "device" else contextlib.nullcontext()):
        step = max(args.batch_pairs, 1) if aligner else 1
        for k in range(0, len(pairs), step):
            group = pairs[k:k + step]
            names = [f"{fx}{args.delim}{fy}" for fx, fy in group]
            gx, gy = [load_mono(fx, args.sr, args.resample) for fx, _ in group], [load_mono(fy, args.sr, args.resample) for _, fy in group]
            if aligner:        # right after loading, before the crop / pad rule (which draws in the list's order either way)
                gx, gy = aligner(gx, gy, names)
            for x, y, name in zip(gx, gy, names):
                x, y, _ = E.crop_or_pad_pair(x, y, target, name=name)
                xs.append(x)
                ys.append(y)
    if aligner:
        print(aligner.summary(), file=sys.stderr)
    res = E.estimate_params(xs, ys, alpha=args.alpha, n_fft=args.nfft, hop=args.hop, qx=args.qx, qrmse=args.qrmse, per_band=args.per_band,
                            batch_pairs=args.batch_pairs, device=f"cuda:{args.device}")
    if args.per_band:
        print(f"Writing resulting per_band sigma_y to {curve_path}", file=sys.stderr)
        np.save(curve_path, res.sigma_y)
    print(f"Writing results to {txt}", file=sys.stderr)
    with open(txt, "w") as f:
        for stream in (out, f):
            print(f"Input pairs file: {os.path.abspath(args.pairs_file)}", file=stream)
            print(f"Args: {args}", file=stream)
            print("=== Results ===", file=stream)
            for line in result_lines(args, res, curve_path):
                print(line, file=stream)
    if args.compare_ckpt:
        ckpt = torch.load(args.compare_ckpt, map_location="cpu", weights_only=False)
        for line in compare_with_ckpt(res, ckpt):
            print(line, file=out)
    return res


def cli(argv=None) -> int:
    run(argv)
    return 0


if __name__ == "__main__":
    sys.exit(cli())
