"""The validation loss of a checkpoint on a list of (clean, coded) pairs, on the GPU: the number the reference's validation_step logs as
`valid_loss` (flowdec/model.py:221-223).

    python -m flowdec_amd.loss_cli --ckpt C --pairs-file P [--target-duration 2] [--no-crop] [--batch 8] [--seed 0]
                                   [--precision bf16|fp32|mixed|bf16x3] [--resample host|device] [--out losses.csv]
                                   [--align MS [--align-frac] [--align-polarity]]

Input: the pair lines of enhance_cli (`clean ---> coded` or `clean,coded`; audio.read_list).  Every file is loaded like eval_cli's:
mean of the channels, resampled to the model's rate when its rate differs.  Each pair then gets the validation set's rule
(data/data_module.py:146-171 with random_crop=False): y is cut to x's length (a y shorter than x is an error), a pair longer than
--target-duration seconds is cropped around its centre (start = int((len - target) / 2)), a shorter one is zero-padded on both sides
(pad // 2 before, pad // 2 + pad % 2 after).  --no-crop keeps every pair at its own length.

The class the checkpoint names runs (checkpoint.model_from_checkpoint).  Pair i of the list is seeded
flowdec_amd.noise.clip_seed(--seed, i): its noise, its time t and therefore its loss do not depend on --batch or on how the pairs were
bucketed.  Prints `valid_loss = ...` (the class's own reduction over all pairs) and, with --out, writes `name,t,loss` per pair.

--align MS [--align-frac] [--align-polarity] [--align-q 64] [--align-taps 32] (off by default; without --align nothing changes): right
after loading and before the length and crop rules, every coded file is aligned against its clean file within +-MS milliseconds -- in
whole samples, with --align-frac on a grid of 1 / Q samples through a windowed-sinc interpolator, with --align-polarity undoing an
inverted polarity -- and both are cut to their common support, on the GPU in batches of --batch (flowdec_amd/align.py: align_pairs; the
switches of eval_cli and estimate_cli).  stdout keeps its text; one alignment summary line and the warnings for a lag at the edge of the
search and an empty support go to stderr."""
import argparse
import contextlib
import os
import sys
from dataclasses import dataclass, field
from typing import List, Optional, Tuple

import numpy as np
import torch

from . import align
from . import loss as fd_loss
from .audio import RESAMPLE_HELP, load_mono, read_list
from .checkpoint import load_from_checkpoint
from .model import RegressionModel, ScoreModel


def crop_or_pad_valid(x: torch.Tensor, y: torch.Tensor, target: int, name: str = "pair") -> Tuple[torch.Tensor, torch.Tensor]:
    """Specs.get(pad_crop=True) of the validation set (data_module.py:146-171, random_crop=False) on the last axis."""
    if x.shape[-1] < y.shape[-1]:
        y = y[..., :x.shape[-1]]
    elif x.shape[-1] > y.shape[-1]:
        raise ValueError(f"{name}: misaligned / broken audio files: y ({y.shape[-1]} samples) cannot be shorter than x ({x.shape[-1]})")
    n = x.shape[-1]
    pad = max(target - n, 0)
    if pad == 0:
        start = int((n - target) / 2)
        return x[..., start:start + target], y[..., start:start + target]
    p = (pad // 2, pad // 2 + pad % 2)
    return torch.nn.functional.pad(x, p), torch.nn.functional.pad(y, p)


def truncate_pair(x: torch.Tensor, y: torch.Tensor, name: str = "pair") -> Tuple[torch.Tensor, torch.Tensor]:
    """--no-crop: only the length rule of data_module.py:146-152."""
    if x.shape[-1] > y.shape[-1]:
        raise ValueError(f"{name}: misaligned / broken audio files: y ({y.shape[-1]} samples) cannot be shorter than x ({x.shape[-1]})")
    return x, y[..., :x.shape[-1]]


@dataclass
class LossResult:
    loss: float = float("nan")
    names: List[str] = field(default_factory=list)
    per_pair: np.ndarray = field(default_factory=lambda: np.zeros(0))
    t: Optional[np.ndarray] = None
    kind: str = "flow"


def model_kind_of(model) -> str:
    return "score" if isinstance(model, ScoreModel) else "regression" if isinstance(model, RegressionModel) else "flow"


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="valid_loss of a FlowDec / ScoreDec / regression checkpoint on (clean, coded) pairs, on MI355X")
    p.add_argument("--ckpt", type=str, required=True)
    p.add_argument("--pairs-file", type=str, required=True, help="lines `clean ---> coded` (or `clean,coded`)")
    p.add_argument("--target-duration", type=float, default=2.0, help="seconds every pair is centre-cropped or zero-padded to")
    p.add_argument("--no-crop", action="store_true", help="keep every pair at its own length")
    p.add_argument("--batch", type=int, default=8, help="pairs per native call")
    p.add_argument("--seed", type=int, default=0, help="pair i is seeded clip_seed(SEED, i)")
    p.add_argument("--precision", type=str, default="bf16", choices=["bf16", "fp32", "mixed", "bf16x3"])
    p.add_argument("--resample", type=str, default="host", choices=["host", "device"], help=RESAMPLE_HELP)
    p.add_argument("--out", type=str, default=None, help="CSV of name,t,loss per pair")
    align.add_pair_arguments(p)
    return p


def load_pairs(args, sr: int, aligner=None):
    """-> (names, xs, ys): the list's pairs, loaded, brought to `sr`, aligned in batches of --batch by `aligner` (--align; None: as they
    are) and cropped / padded by the validation set's rule."""
    fl = read_list(args.pairs_file)
    if not fl.from_pairs or not fl.inputs:
        raise ValueError(f"{args.pairs_file}: no `clean ---> coded` pair lines")
    target = int(args.target_duration * sr)
    files = [(fx.strip(), fy.strip()) for fx, fy in zip(fl.clean, fl.inputs)]
    step = max(args.batch, 1) if aligner else 1
    names, xs, ys = [], [], []
    for k in range(0, len(files), step):
        group = files[k:k + step]
        full = [f"{fx} ---> {fy}" for fx, fy in group]
        gx, gy = [load_mono(fx, sr, args.resample) for fx, _ in group], [load_mono(fy, sr, args.resample) for _, fy in group]
        if aligner:
            gx, gy = aligner(gx, gy, full)
        for (_, fy), x, y, name in zip(group, gx, gy, full):
            x, y = truncate_pair(x, y, name) if args.no_crop else crop_or_pad_valid(x, y, target, name)
            names.append(os.path.basename(fy)); xs.append(x); ys.append(y)
    return names, xs, ys


def write_csv(path: str, res: LossResult) -> None:
    with open(path, "w") as f:
        f.write("name,t,loss\n")
        for i, n in enumerate(res.names):
            t = "" if res.t is None else repr(float(res.t[i]))
            f.write(f"{n},{t},{float(res.per_pair[i])!r}\n")


def run(argv=None, model=None, out=None) -> LossResult:
    """`model`: an already built model (tests); otherwise the checkpoint's."""
    out = out or sys.stdout
    parser = build_parser()
    args = parser.parse_args(list(sys.argv[1:] if argv is None else argv))
    if (args.align_frac or args.align_polarity) and args.align is None:
        parser.error("--align-frac and --align-polarity need --align MS")
    if model is None:
        model = load_from_checkpoint(args.ckpt, map_location="cuda", precision=args.precision)
    kind = model_kind_of(model)
    aligner = None
    if args.align is not None:
        try:
            aligner = align.PairAligner(args, int(model.sampling_rate), args.batch, device=model.device)
        except ValueError as err:
            parser.error(str(err))
    with (torch.cuda.device(model.device) if args.resample == "device" else contextlib.nullcontext()):
        names, xs, ys = load_pairs(args, int(model.sampling_rate), aligner)
    if aligner:
        print(aligner.summary(), file=sys.stderr)
    kw = {} if kind == "regression" else dict(seeds=int(args.seed), return_t=True)
    got = model.valid_loss_batch(xs, ys, reduce="none", max_batch=args.batch, **kw)
    values, t = got if kind != "regression" else (got, None)
    res = LossResult(loss=fd_loss.reduce_values(kind, values, names), names=names, per_pair=np.asarray(values), t=None if t is None else np.asarray(t),
                     kind=kind)
    print(f"valid_loss = {res.loss!r}   ({kind}, {len(names)} pairs, precision {args.precision}, seed {args.seed})", file=out)
    if args.out:
        write_csv(args.out, res)
    return res


def cli(argv=None) -> int:
    run(argv)
    return 0


if __name__ == "__main__":
    sys.exit(cli())
