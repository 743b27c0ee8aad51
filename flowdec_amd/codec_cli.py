"""Pipe front end of the streaming NDAC encoder: raw PCM in, code indices out, written as they become final.

    python -m flowdec_amd.codec_cli --codec WEIGHTS.pth --format s16le|f32le [--n-quantizers Q] [--encode-block-frames 8] \\
        [--in - --out -] [--block-samples 4800]

The input is mono PCM, little endian, without a header, at the codec's sampling rate (there is no resampling here).  The output is the
stream `stream_cli --codes` reads: little-endian int16, frame-major, Q values per frame (Q = --n-quantizers, default: all of the
codec's codebooks).  Concatenated it is `dac.encode(dac.preprocess(input), Q)[1][0]` bit for bit, however the pipe cut the input
(`ndac_stream.EncodeStream` on the codec `DAC.load(WEIGHTS.pth)`); a trailing partial frame is zero-padded, as `preprocess` pads it.
s16le input is x / 32768.  A frame's codes leave once (block_frames + halo_right - 1) * hop further samples have arrived, plus one
window's compute time; the delay is reported on stderr.  There is no decode mode: `stream_cli --codes` is the decoder."""
import argparse
import sys
from typing import List, Optional

import numpy as np
import torch

from .ndac import DAC
from .ndac_stream import EncodeStream

FORMATS = {"s16le": np.dtype("<i2"), "f32le": np.dtype("<f4")}
INT16_CODES = 1 << 15          # code indices [0, 32768) fit the int16 stream


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="Encode a raw PCM stream to NDAC code indices on MI355X (stdin -> stdout by default)")
    p.add_argument("--codec", type=str, required=True, help="NDAC weights.pth (DAC.load)")
    p.add_argument("--format", type=str, required=True, choices=sorted(FORMATS), help="sample format of the input")
    p.add_argument("--n-quantizers", type=int, default=None, help="code indices per frame (default: all of the codec's codebooks)")
    p.add_argument("--encode-block-frames", type=int, default=8, help="frames the streaming encoder emits at a time")
    p.add_argument("--in", dest="inp", type=str, default="-", help="input file (default -: stdin)")
    p.add_argument("--out", type=str, default="-", help="output file (default -: stdout)")
    p.add_argument("--block-samples", type=int, default=4800, help="samples read per push")
    p.add_argument("--device", type=str, default="cuda:0")
    p.add_argument("--precision", type=str, default="mfma_decoder", choices=sorted(DAC.PRECISIONS),
                   help="mfma_decoder / exact: the exact encoder (code indices reproducible); mfma: the encoder on the matrix cores")
    return p


def parse_args(argv: Optional[List[str]] = None) -> argparse.Namespace:
    p = build_parser()
    args = p.parse_args(argv)
    if args.block_samples < 1:
        p.error("--block-samples must be >= 1")
    if args.n_quantizers is not None and args.n_quantizers < 1:
        p.error("--n-quantizers must be >= 1")
    if args.encode_block_frames < 1:
        p.error("--encode-block-frames must be >= 1")
    return args


def decode_pcm(buf: bytes, fmt: str) -> torch.Tensor:
    """Whole samples of `fmt` -> float32 (s16le: x / 32768)."""
    a = np.frombuffer(buf, dtype=FORMATS[fmt])
    return torch.from_numpy(a.astype(np.float32) / np.float32(32768.0) if fmt == "s16le" else a.astype(np.float32))


def code_bytes(codes: torch.Tensor) -> bytes:
    """[nq, k] codes -> the bytes of k frames of the int16 stream: frame-major, nq values per frame, little endian."""
    a = codes.detach().to("cpu").numpy()
    if a.size and (a.min() < 0 or a.max() >= INT16_CODES):
        raise ValueError(f"code_bytes: a code outside [0, {INT16_CODES}) does not fit the int16 stream")
    return np.ascontiguousarray(a.T).astype("<i2").tobytes()


def run(argv: Optional[List[str]] = None, dac=None) -> int:
    """-> the number of frames written.  `dac`: an already loaded DAC (tests)."""
    args = parse_args(argv)
    error = build_parser().error
    if dac is None:
        dac = DAC.load(args.codec, precision=args.precision).to(args.device)
    if dac.codebook_size > INT16_CODES:
        error(f"--codec: a codebook of {dac.codebook_size} entries does not fit the int16 code stream (at most {INT16_CODES})")
    nq = dac.n_codebooks if args.n_quantizers is None else args.n_quantizers
    if nq > dac.n_codebooks:
        error(f"--n-quantizers {nq}: the codec has {dac.n_codebooks} codebooks")
    st = EncodeStream(dac, n_quantizers=nq, block_frames=args.encode_block_frames)
    dt = FORMATS[args.format]
    fin = sys.stdin.buffer if args.inp == "-" else open(args.inp, "rb")
    fout = sys.stdout.buffer if args.out == "-" else open(args.out, "wb")
    frames = 0
    try:
        rest = b""
        while True:
            buf = fin.read(args.block_samples * dt.itemsize)
            if not buf:
                break
            buf = rest + buf
            k = len(buf) // dt.itemsize * dt.itemsize            # a pipe may cut a sample in two
            buf, rest = buf[:k], buf[k:]
            if not buf:
                continue
            c = st.push(decode_pcm(buf, args.format))
            if c.shape[1]:
                fout.write(code_bytes(c))
                fout.flush()
                frames += c.shape[1]
        if rest:
            print(f"codec_cli: {len(rest)} trailing bytes are not a whole sample: dropped", file=sys.stderr)
        c = st.flush()
        fout.write(code_bytes(c))
        fout.flush()
        frames += c.shape[1]
    finally:
        if fin is not sys.stdin.buffer:
            fin.close()
        if fout is not sys.stdout.buffer:
            fout.close()
    print(f"codec_cli: {frames} frames of {nq} codes written ({st.samples_received} samples in; delay {st.delay_samples} samples at "
          f"{dac.sample_rate} Hz = {1e3 * st.delay_samples / dac.sample_rate:.2f} ms; {st.windows_run} windows, {st.frames_encoded} frames encoded)",
          file=sys.stderr)
    return frames


def main(argv=None) -> int:
    run(argv)
    return 0


if __name__ == "__main__":
    sys.exit(main())
