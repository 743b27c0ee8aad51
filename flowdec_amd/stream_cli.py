"""Pipe front end of the streaming enhancer: raw PCM in, raw PCM out, written as it becomes final.

    python -m flowdec_amd.stream_cli --ckpt C --N 6 --solver euler --seed 7 [--row-frames 256 --halo-frames 64] \\
        --normfac causal|FLOAT --format s16le|f32le [--in - --out -] [--block-samples 4800] [--in-rate R] [--out-rate R]

The checkpoint names the model class (flowdec_amd.checkpoint): a FlowDec checkpoint runs as above; a ScoreDec checkpoint takes --N and, in
place of --solver, --predictor / --corrector / --corrector-steps / --snr (its predictor-corrector sampler); a regression checkpoint makes one
network evaluation per row and ignores --N, --solver and --seed (it says so on stderr).  --codes works with all three.

The input is mono PCM, little endian, without a header, at the model's sampling rate unless --in-rate says otherwise.  The output -- same
format -- is, as float32, the model's long-form enhance of the input (`enhance_long(input, seed=SEED, normfac=..., row_frames=...,
halo_frames=...)`) bit for bit (flowdec_amd.stream); s16le output is that rounded to 16 bits with clipping.  A sample leaves once (row_frames - halo_frames) * hop +
xfade / 2 further samples have arrived, plus one row's compute time.

--in-rate / --out-rate (default: the model's rate) resample the stream on the device on its way in and out (flowdec_amd.resample:
torchaudio's sinc resampler at lowpass_filter_width 64, stateful, independent of the cut into blocks): the float32 output is then
resample_device(enhance_long(resample_device(input, IN, model rate)), model rate, OUT) bit for bit.  Each resampler adds width + o
samples of delay at its own input rate; the line on stderr reports the three delays.

    python -m flowdec_amd.stream_cli --codes --codec WEIGHTS.pth [--n-quantizers Q] [--decode-block-frames 8] --ckpt C ... --format f32le

--codes: the input is a headerless stream of NDAC code indices instead of PCM -- little-endian int16, frame-major, Q values per frame
(Q = --n-quantizers, default: all of the codec's codebooks); a pipe may cut a frame in two.  The frames go through
`ndac_stream.DecodeStream` on the codec `DAC.load(WEIGHTS.pth)` and from there into the enhancer; the codec's sampling rate takes the
place of --in-rate, and --format names the output only.  The float32 output equals this program fed the one-shot decoded PCM
(`dac.decode(dac.quantizer.from_codes(codes)[0])`) as f32le, byte for byte.  The decoder adds (block_frames + halo_right - 1) * hop samples
of delay at the codec's rate, reported on stderr with the others."""
import argparse
import sys
from typing import List, Optional

import numpy as np
import torch

from .checkpoint import load_from_checkpoint
from .model import RegressionModel, ScoreModel
from .ndac import DAC
from .ndac_stream import DecodeStream
from .stream import EnhanceStream

FORMATS = {"s16le": np.dtype("<i2"), "f32le": np.dtype("<f4")}


def _normfac(s: str):
    if s == "causal":
        return s
    try:
        v = float(s)
    except ValueError:
        raise argparse.ArgumentTypeError(f"--normfac is 'causal' or a positive number (got {s!r})")
    if not (np.isfinite(v) and v > 0):
        raise argparse.ArgumentTypeError(f"--normfac is 'causal' or a positive number (got {s!r})")
    return v


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="Enhance a raw PCM stream with a FlowDec, ScoreDec or regression postfilter on MI355X (stdin -> stdout by default).  The output is "
                                            "not loudness-normalised: a stream has no integrated loudness until it ends (enhance_cli --target-lufs "
                                            "sets the level of files)")
    p.add_argument("--ckpt", type=str, required=True)
    p.add_argument("--N", type=int, required=True)
    p.add_argument("--solver", type=str, default="euler", choices=["euler", "midpoint", "heun2", "heun2_eulerlast"], help="flow checkpoint: fixed-step solvers only")
    p.add_argument("--predictor", type=str, default="reverse_diffusion", choices=["reverse_diffusion", "euler_maruyama", "none"], help="score checkpoint")
    p.add_argument("--corrector", type=str, default="ald", choices=["ald", "none"], help="score checkpoint")
    p.add_argument("--corrector-steps", type=int, default=1, help="score checkpoint")
    p.add_argument("--snr", type=float, default=0.5, help="score checkpoint: the corrector's target SNR")
    p.add_argument("--seed", type=int, required=True, help="the stream's noise seed, as enhance_long(seed=SEED)")
    p.add_argument("--row-frames", type=int, default=256, help="STFT frames per row (a multiple of 64)")
    p.add_argument("--halo-frames", type=int, default=64)
    p.add_argument("--normfac", type=_normfac, required=True,
                   help="causal: every row is scaled by the peak of the stream up to its end; FLOAT: a fixed factor (full scale: 1.0)")
    p.add_argument("--format", type=str, required=True, choices=sorted(FORMATS))
    p.add_argument("--in", dest="inp", type=str, default="-", help="input file (default -: stdin)")
    p.add_argument("--out", type=str, default="-", help="output file (default -: stdout)")
    p.add_argument("--block-samples", type=int, default=4800, help="samples read per push")
    p.add_argument("--in-rate", type=int, default=None, help="sampling rate of the input in Hz (default: the model's rate)")
    p.add_argument("--out-rate", type=int, default=None, help="sampling rate of the output in Hz (default: the model's rate)")
    p.add_argument("--codes", action="store_true", help="the input is int16 NDAC code indices (frame-major, Q per frame), decoded by --codec")
    p.add_argument("--codec", type=str, default=None, help="NDAC weights.pth (DAC.load) that decodes the --codes stream")
    p.add_argument("--n-quantizers", type=int, default=None, help="code indices per frame (default: all of the codec's codebooks)")
    p.add_argument("--decode-block-frames", type=int, default=8, help="frames the streaming decoder emits at a time")
    p.add_argument("--device", type=str, default="cuda:0")
    p.add_argument("--ema", type=lambda s: str(s).lower() not in ("0", "false", "no"), default=True)
    p.add_argument("--precision", type=str, default="bf16", choices=["bf16", "fp32", "mixed", "bf16x3"])
    return p


def parse_args(argv: Optional[List[str]] = None) -> argparse.Namespace:
    p = build_parser()
    args = p.parse_args(argv)
    if args.block_samples < 1:
        p.error("--block-samples must be >= 1")
    if args.N < 1:
        p.error("--N must be >= 1")
    if args.corrector_steps < 0:
        p.error("--corrector-steps must be >= 0")
    for name in ("in_rate", "out_rate"):
        if getattr(args, name) is not None and getattr(args, name) < 1:
            p.error(f"--{name.replace('_', '-')} must be >= 1")
    if args.codes and not args.codec:
        p.error("--codes needs --codec WEIGHTS.pth (the NDAC codec that decodes the stream)")
    if args.codec and not args.codes:
        p.error("--codec is the decoder of a --codes stream; without --codes the input is PCM")
    if args.n_quantizers is not None and not args.codes:
        p.error("--n-quantizers belongs to --codes")
    if args.n_quantizers is not None and args.n_quantizers < 1:
        p.error("--n-quantizers must be >= 1")
    if args.decode_block_frames < 1:
        p.error("--decode-block-frames must be >= 1")
    return args


class CodeFrames:
    """Bytes of a --codes stream -> whole frames.  `feed(buf)` returns the frames the bytes so far complete as an int64 array [nq, n]
    (possibly n = 0) and carries a cut frame over to the next call; a code outside [0, codebook_size) goes to `error` (the parser's:
    exits) with the index of its frame in the stream."""

    def __init__(self, nq: int, codebook_size: int, error):
        self.nq, self.codebook_size, self.error = int(nq), int(codebook_size), error
        self.rest, self.frames = b"", 0

    def feed(self, buf: bytes) -> np.ndarray:
        buf = self.rest + buf
        k = len(buf) // (2 * self.nq) * (2 * self.nq)
        buf, self.rest = buf[:k], buf[k:]
        a = np.frombuffer(buf, dtype="<i2").astype(np.int64).reshape(-1, self.nq)
        bad = np.nonzero(((a < 0) | (a >= self.codebook_size)).any(axis=1))[0]
        if bad.size:
            f = int(bad[0])
            self.error(f"--codes: frame {self.frames + f} holds the code {int(a[f][(a[f] < 0) | (a[f] >= self.codebook_size)][0])}, outside "
                       f"[0, {self.codebook_size})")
        self.frames += a.shape[0]
        return np.ascontiguousarray(a.T)


def encode(x: torch.Tensor, fmt: str) -> bytes:
    """float32 samples -> the bytes of `fmt` (s16le: round(x * 32768) clipped to [-32768, 32767])."""
    a = x.detach().to("cpu", torch.float32).numpy()
    if fmt == "s16le":
        a = np.clip(np.rint(a.astype(np.float64) * 32768.0), -32768, 32767)
    return a.astype(FORMATS[fmt]).tobytes()


def run(argv: Optional[List[str]] = None, model=None) -> int:
    """-> the number of samples written.  `model`: an already loaded FlowModel, ScoreModel or RegressionModel (tests)."""
    args = parse_args(argv)
    if model is None:
        model = load_from_checkpoint(args.ckpt, map_location=args.device, ema=args.ema, precision=args.precision)   # the class the checkpoint names
    if isinstance(model, RegressionModel):
        print("stream_cli: a regression checkpoint makes one network evaluation per row: --N, --solver and --seed are ignored", file=sys.stderr)
        sampler = dict(seed=None)
    elif isinstance(model, ScoreModel):
        sampler = dict(seed=args.seed, N=args.N, predictor=args.predictor, corrector=args.corrector, corrector_steps=args.corrector_steps, snr=args.snr)
    else:
        sampler = dict(seed=args.seed, N=args.N, solver=args.solver)
    dec = split = None
    if args.codes:
        error = build_parser().error
        dac = DAC.load(args.codec).to(model.device)
        nq = dac.n_codebooks if args.n_quantizers is None else args.n_quantizers
        if nq > dac.n_codebooks:
            error(f"--n-quantizers {nq}: the codec has {dac.n_codebooks} codebooks")
        if args.in_rate is not None and args.in_rate != dac.sample_rate:
            error(f"--in-rate {args.in_rate}: a --codes stream decodes to the codec's rate, {dac.sample_rate} Hz")
        if dac.sample_rate != model.sampling_rate:
            args.in_rate = int(dac.sample_rate)
        dec = DecodeStream(dac, n_quantizers=nq, block_frames=args.decode_block_frames)
        split = CodeFrames(nq, dac.codebook_size, error)
    st = EnhanceStream(model, row_frames=args.row_frames, halo_frames=args.halo_frames, normfac=args.normfac, in_rate=args.in_rate,
                       out_rate=args.out_rate, **sampler)
    dt = FORMATS[args.format]
    fin = sys.stdin.buffer if args.inp == "-" else open(args.inp, "rb")
    fout = sys.stdout.buffer if args.out == "-" else open(args.out, "wb")
    written = 0
    try:
        want = args.block_samples * (2 if split else dt.itemsize)
        rest = b""
        while True:
            buf = fin.read(want)
            if not buf:
                break
            if split:          # code frames -> decoded PCM -> the enhancer
                frames = split.feed(buf)
                x = dec.push(torch.from_numpy(frames)) if frames.shape[1] else None
                if x is None or not x.numel():
                    continue
                y = st.push(x)
                if y.numel():
                    fout.write(encode(y, args.format))
                    fout.flush()
                    written += y.numel()
                continue
            buf = rest + buf
            k = len(buf) // dt.itemsize * dt.itemsize            # a pipe may cut a sample in two
            buf, rest = buf[:k], buf[k:]
            if not buf:
                continue
            y = st.push(torch.from_numpy(np.frombuffer(buf, dtype=dt).astype(dt.newbyteorder("=")).copy()))
            if y.numel():
                fout.write(encode(y, args.format))
                fout.flush()
                written += y.numel()
        if split:
            if split.rest:
                print(f"stream_cli: {len(split.rest)} trailing bytes are not a whole frame of {split.nq} codes: dropped", file=sys.stderr)
            x = dec.flush()
            if x.numel():
                y = st.push(x)
                fout.write(encode(y, args.format))
                written += y.numel()
        y = st.flush()
        fout.write(encode(y, args.format))
        fout.flush()
        written += y.numel()
    finally:
        if fin is not sys.stdin.buffer:
            fin.close()
        if fout is not sys.stdout.buffer:
            fout.close()
    sr = model.sampling_rate
    d_in, d_pool, d_out = st.delays
    print(f"stream_cli: {written} samples written (delay {st.delay_samples} samples; resampler in {d_in} samples at {st.in_rate} Hz = "
          f"{1e3 * d_in / st.in_rate:.2f} ms, pool {d_pool} samples at {sr} Hz = {1e3 * d_pool / sr:.2f} ms, resampler out {d_out} samples at {sr} Hz = "
          f"{1e3 * d_out / sr:.2f} ms" + (f", decoder {dec.delay_samples} samples at {dec.dac.sample_rate} Hz = "
                                           f"{1e3 * dec.delay_samples / dec.dac.sample_rate:.2f} ms" if dec else "") + ")", file=sys.stderr)
    return written


def main(argv=None) -> int:
    run(argv)
    return 0


if __name__ == "__main__":
    sys.exit(main())
