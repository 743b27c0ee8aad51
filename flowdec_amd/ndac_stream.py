"""Streaming and long-form NDAC decode: codes in, PCM out, bit for bit `dac.decode(dac.quantizer.from_codes(all codes)[0])`.

Every decoder layer has a finite receptive field, and every kernel accumulates an output in an order that does not depend on the
output's position (csrc/ndac_conv1d.hip: input channels ascending, taps ascending, then the bias; the transposed convolution's tap phase is
(n + p) mod s, which a shift by whole frames leaves alone; csrc/ndac_mfma.hip: the K order of an output is the same in every tile
variant).  So a WINDOW of frames with `DAC.decode_halo()` = (left, right) frames of real context on both sides -- or a true edge of the
signal, where the window's zero padding IS the signal's -- reproduces the bits of the one-shot decode on its interior (DESIGN.md
section 2 "Streaming decode").

`DecodePlanner` (host only) decides which frames can leave and which window decodes them; `DecodeStream` is the push / flush session
on a `flowdec_amd.ndac.DAC`; `decode_long` runs the same jobs over a finished recording through one fixed workspace.  Cost: every
emitted block of b frames decodes b + left + right frames, a recompute share of (b + left + right) / b.

The other direction -- samples in, codes out, bit for bit `dac.encode(dac.preprocess(all samples))[1]` -- is `EncodeStream` and
`encode_long` at the end of this file, on the same planner with `DAC.encode_halo()` (DESIGN.md section 2 "Streaming encode").
"""
from typing import List, Optional, Tuple

import torch

Job = Tuple[int, int, int, int]   # (win_start, win_end, emit_start, emit_end) in absolute frames


class DecodePlanner:
    """Which frames are final, and the window that decodes them.  Host only.

    Frames [e, e + k * block) leave as soon as `received >= e + k * block + halo_right` (k as large as possible), one job per block;
    `flush` emits what is left as one job.  A job's window is [max(0, emit_start - halo_left), min(received, emit_end + halo_right)).
    A frame has left once at most `latency_frames` = block + halo_right - 1 further frames have arrived, and between pushes no more than
    `max_buffered` = halo_left + block + halo_right - 1 frames have to be kept (`keep_from` .. `received`)."""

    def __init__(self, halo_left: int, halo_right: int, block_frames: int):
        if int(halo_left) < 0 or int(halo_right) < 0:
            raise ValueError(f"DecodePlanner: halos must be >= 0 (got {halo_left}, {halo_right})")
        if int(block_frames) < 1:
            raise ValueError(f"DecodePlanner: block_frames must be >= 1 (got {block_frames})")
        self.halo_left, self.halo_right, self.block = int(halo_left), int(halo_right), int(block_frames)
        self.received = self.emitted = 0
        self.closed = False
        self.latency_frames = self.block + self.halo_right - 1
        self.max_buffered = self.halo_left + self.block + self.halo_right - 1

    @property
    def keep_from(self) -> int:
        """The first frame a later job can still ask for."""
        return max(0, self.emitted - self.halo_left)

    @property
    def buffered(self) -> int:
        return self.received - self.keep_from

    def _job(self, e0: int, e1: int) -> Job:
        return (max(0, e0 - self.halo_left), min(self.received, e1 + self.halo_right), e0, e1)

    def push(self, n_frames: int) -> List[Job]:
        if self.closed:
            raise RuntimeError("DecodePlanner: push after flush")
        if int(n_frames) < 0:
            raise ValueError(f"DecodePlanner: n_frames must be >= 0 (got {n_frames})")
        self.received += int(n_frames)
        jobs = []
        while self.received >= self.emitted + self.block + self.halo_right:
            jobs.append(self._job(self.emitted, self.emitted + self.block))
            self.emitted += self.block
        return jobs

    def flush(self) -> List[Job]:
        if self.closed:
            raise RuntimeError("DecodePlanner: flush after flush")
        self.closed = True
        if self.emitted == self.received:
            return []
        job = self._job(self.emitted, self.received)
        self.emitted = self.received
        return [job]


def _as_code_rows(codes, who: str) -> torch.Tensor:
    """[nq, n] or [1, nq, n] integer codes -> [nq, n]."""
    if not isinstance(codes, torch.Tensor) or codes.dtype.is_floating_point or codes.dtype in (torch.bool, torch.complex64, torch.complex128):
        raise TypeError(f"{who}: codes must be an integer tensor")
    if codes.ndim == 3 and codes.shape[0] == 1:
        codes = codes[0]
    if codes.ndim != 2:
        raise RuntimeError(f"{who}: codes must be [nq, n] or [1, nq, n] (got {tuple(codes.shape)})")
    return codes


def _samples_per_frame(dac) -> int:
    """Decoded samples per latent frame (even decoder rates: T frames decode to T times this)."""
    up = 1
    for s in dac.decoder_rates:
        up *= int(s)
    return up


def _run_jobs(dac, window_codes: List[torch.Tensor], jobs: List[Job], rows_per_call: int, ws=None) -> List[torch.Tensor]:
    """window_codes[i]: the [nq, win_end - win_start] device codes of jobs[i] -> its final samples, 1-D.  `rows_per_call` jobs share one
    ragged decode; a lone job without a caller's workspace is a plain decode of its window (the same bits: a ragged row IS its one-clip
    decode)."""
    hop, outs = _samples_per_frame(dac), []
    for g in range(0, len(jobs), rows_per_call):
        grp, wc = jobs[g:g + rows_per_call], window_codes[g:g + rows_per_call]
        if len(grp) == 1 and ws is None:
            y = dac.decode(dac.quantizer.from_codes(wc[0][None])[0])
        else:
            T = max(c.shape[1] for c in wc)
            rows = torch.zeros(len(grp), wc[0].shape[0], T, dtype=wc[0].dtype, device=wc[0].device)   # (code 0 behind a window: never read as data)
            for b, c in enumerate(wc):
                rows[b, :, :c.shape[1]] = c
            y = dac.decode_ragged(dac.quantizer.from_codes(rows)[0], [c.shape[1] for c in wc], ws=ws)
        for b, (w0, _, e0, e1) in enumerate(grp):
            outs.append(y[b, 0, (e0 - w0) * hop:(e1 - w0) * hop])
    return outs


class DecodeStream:
    """One streaming decode session on a `DAC` (on the GPU, even decoder rates).

        st = DecodeStream(dac, block_frames=8)
        for packet in packets: out.append(st.push(packet))     # [nq, n] integer codes, any n >= 0, host or device
        out.append(st.flush())         # torch.cat(out) == dac.decode(dac.quantizer.from_codes(cat(packets)[None])[0])[0, 0], bit for bit

    however the codes were cut into pushes, for every block_frames >= 1 and in both precisions.  `n_quantizers`: the code rows per
    frame (None: the first push decides; at most the model's codebooks, as `quantizer.from_codes` demands).  A push that finishes several
    blocks decodes them as rows of ragged calls, `rows_per_call` at a time.  `delay_samples`: a sample leaves once that many further
    samples' frames have arrived, plus one window's compute time."""

    def __init__(self, dac, n_quantizers: Optional[int] = None, block_frames: int = 8, rows_per_call: int = 4):
        if dac.device.type != "cuda":
            raise RuntimeError("flowdec_amd.ndac: the codec must be on the GPU (`dac_model.to('cuda')`); there is no CPU path")
        if int(rows_per_call) < 1:
            raise ValueError(f"DecodeStream: rows_per_call must be >= 1 (got {rows_per_call})")
        if n_quantizers is not None and not 1 <= int(n_quantizers) <= dac.n_codebooks:
            raise RuntimeError(f"DecodeStream: {n_quantizers} code rows but the model has {dac.n_codebooks} codebooks")
        self.dac, self.nq, self.rows_per_call = dac, None if n_quantizers is None else int(n_quantizers), int(rows_per_call)
        left, right = dac.decode_halo()
        self.planner = DecodePlanner(left, right, block_frames)
        self.delay_samples = self.planner.latency_frames * _samples_per_frame(dac)
        self._codes = None      # [nq, buffered] device codes, column 0 = absolute frame self._base
        self._base = 0
        self.windows_run = self.frames_decoded = 0

    @property
    def buffered_frames(self) -> int:
        return 0 if self._codes is None else int(self._codes.shape[1])

    def _empty(self) -> torch.Tensor:
        return torch.empty(0, dtype=torch.float32, device=self.dac.device)

    def _run(self, jobs: List[Job]) -> torch.Tensor:
        if jobs:
            wc = [self._codes[:, w0 - self._base:w1 - self._base] for w0, w1, _, _ in jobs]
            outs = _run_jobs(self.dac, wc, jobs, self.rows_per_call)
            self.windows_run += len(jobs)
            self.frames_decoded += sum(w1 - w0 for w0, w1, _, _ in jobs)
            y = torch.cat(outs)
        else:
            y = self._empty()
        keep = self.planner.keep_from          # only the codes the planner can still ask for stay
        if self._codes is not None and keep > self._base:
            self._codes = self._codes[:, keep - self._base:].clone()
            self._base = keep
        return y

    def push(self, codes) -> torch.Tensor:
        """-> the samples that became final (float32, 1-D, on the codec's device; possibly empty)."""
        c = _as_code_rows(codes, "DecodeStream.push")
        if self.nq is None:
            if not 1 <= c.shape[0] <= self.dac.n_codebooks:
                raise RuntimeError(f"DecodeStream.push: {c.shape[0]} code rows but the model has {self.dac.n_codebooks} codebooks")
            self.nq = int(c.shape[0])
        if c.shape[0] != self.nq:
            raise RuntimeError(f"DecodeStream.push: {c.shape[0]} code rows, the stream has {self.nq}")
        if self.planner.closed:
            raise RuntimeError("DecodeStream: push after flush")
        c = c.to(self.dac.device, torch.int64)
        self._codes = c.clone() if self._codes is None else torch.cat([self._codes, c], dim=1)
        return self._run(self.planner.push(c.shape[1]))

    def flush(self) -> torch.Tensor:
        """-> the rest of the stream; ends the session."""
        y = self._run(self.planner.flush())
        self._codes = None
        return y


def decode_long(dac, codes, window_frames: int = 1024, rows_per_call: int = 4) -> torch.Tensor:
    """codes [nq, T] or [1, nq, T] -> audio [1, 1, L], bit for bit `dac.decode(dac.quantizer.from_codes(codes)[0])`, through windows of at
    most `window_frames` frames, `rows_per_call` of them per ragged call, in ONE workspace sized for (rows_per_call, window_frames)
    whatever T.  A recording that fits one window is one plain decode call."""
    c = _as_code_rows(codes, "decode_long")
    if dac.device.type != "cuda":
        raise RuntimeError("flowdec_amd.ndac: the codec must be on the GPU (`dac_model.to('cuda')`); there is no CPU path")
    if int(rows_per_call) < 1:
        raise ValueError(f"decode_long: rows_per_call must be >= 1 (got {rows_per_call})")
    if not 1 <= c.shape[0] <= dac.n_codebooks:
        raise RuntimeError(f"decode_long: {c.shape[0]} code rows but the model has {dac.n_codebooks} codebooks")
    if c.shape[1] < 1:
        raise RuntimeError("decode_long: no frames")
    c = c.to(dac.device, torch.int64)
    window_frames, rows_per_call, T = int(window_frames), int(rows_per_call), int(c.shape[1])
    if T <= window_frames:
        return dac.decode(dac.quantizer.from_codes(c[None])[0])
    left, right = dac.decode_halo()
    if window_frames <= left + right:
        raise ValueError(f"decode_long: window_frames must exceed the decoder's halos {left} + {right} (got {window_frames})")
    planner = DecodePlanner(left, right, window_frames - left - right)
    jobs = planner.push(T) + planner.flush()
    ws = dac.decode_workspace(rows_per_call, window_frames)
    hop = _samples_per_frame(dac)
    out = torch.empty(1, 1, T * hop, dtype=torch.float32, device=dac.device)
    for g in range(0, len(jobs), rows_per_call):
        grp = jobs[g:g + rows_per_call]
        ys = _run_jobs(dac, [c[:, w0:w1] for w0, w1, _, _ in grp], grp, rows_per_call, ws=ws)
        for (_, _, e0, e1), y in zip(grp, ys):
            out[0, 0, e0 * hop:e1 * hop] = y
    return out


# ---- streaming and long-form ENCODE: samples in, codes out -----------------------------------------------------------------------------
# The same premise on the other side of the codec: every encoder layer has a finite receptive field and a per-output operation order that
# does not depend on position (a strided convolution's phase is kept by a shift of whole frames, odd strides included), so a window of whole
# hops with `DAC.encode_halo()` = (left, right) frames of real samples on both sides -- or a true edge of the signal -- reproduces the
# one-shot encoder output on its interior frames bit for bit, and the quantiser works per frame.  DecodePlanner is reused unchanged with
# frames received = complete hops of samples.


def _run_encode_jobs(dac, windows: List[torch.Tensor], jobs: List[Job], nq: Optional[int], rows_per_call: int, ws=None):
    """windows[i]: the (win_end - win_start) * hop device samples of jobs[i], 1-D -> per job (z [D, k], codes [nq, k], latents [nq * cd, k])
    of its final frames.  `rows_per_call` jobs share one ragged encode; a lone job is a ragged call of one row (the same bits as the
    plain encode of its window -- a ragged row IS its one-clip encode -- with the quantiser as one launch instead of one per codebook)."""
    hop, outs = dac.hop_length, []
    for g in range(0, len(jobs), rows_per_call):
        grp, wx = jobs[g:g + rows_per_call], windows[g:g + rows_per_call]
        rows = torch.zeros(len(grp), 1, max(x.numel() for x in wx), dtype=torch.float32, device=wx[0].device)
        for b, x in enumerate(wx):
            rows[b, 0, :x.numel()] = x
        z, codes, lat = dac.encode_ragged(rows, [x.numel() // hop for x in wx], nq, ws=ws)
        for b, (w0, _, e0, e1) in enumerate(grp):
            outs.append((z[b, :, e0 - w0:e1 - w0], codes[b, :, e0 - w0:e1 - w0], lat[b, :, e0 - w0:e1 - w0]))
    return outs


class EncodeStream:
    """One streaming encode session on a `DAC` (on the GPU).

        st = EncodeStream(dac, n_quantizers=4, block_frames=8)
        for chunk in chunks: out.append(st.push(chunk))     # float32 samples, 1-D, any length >= 0, host or device
        out.append(st.flush())    # torch.cat(out, 1) == dac.encode(dac.preprocess(cat(chunks)[None, None]), 4)[1][0], bit for bit

    however the samples were cut into pushes, for every block_frames >= 1 and in both precisions.  `push` returns the [nq, k] int64 codes
    that became final (possibly k = 0); `flush` zero-pads a trailing partial frame, as `preprocess` does, and ends the session.  Only
    codes leave: `from_codes(codes)` is not bitwise the encoder's straight-through z.  A push that finishes several blocks encodes them as
    rows of ragged calls, `rows_per_call` at a time.  `delay_samples`: a frame's codes leave once that many further samples have arrived,
    plus one window's compute time."""

    def __init__(self, dac, n_quantizers: Optional[int] = None, block_frames: int = 8, rows_per_call: int = 4):
        if int(rows_per_call) < 1:
            raise ValueError(f"EncodeStream: rows_per_call must be >= 1 (got {rows_per_call})")
        if n_quantizers is not None and not 1 <= int(n_quantizers) <= dac.n_codebooks:
            raise RuntimeError(f"EncodeStream: {n_quantizers} code rows but the model has {dac.n_codebooks} codebooks")
        self.dac, self.rows_per_call = dac, int(rows_per_call)
        self.nq = dac.n_codebooks if n_quantizers is None else int(n_quantizers)
        left, right = dac.encode_halo()
        self.planner = DecodePlanner(left, right, block_frames)
        self.hop = int(dac.hop_length)
        self.delay_samples = self.planner.latency_frames * self.hop
        self._x = torch.empty(0, dtype=torch.float32, device=dac.device)   # buffered samples, element 0 = absolute sample self._base
        self._base = 0
        self.samples_received = 0
        self.windows_run = self.frames_encoded = 0

    @property
    def buffered_samples(self) -> int:
        return int(self._x.numel())

    def _run(self, jobs: List[Job]) -> torch.Tensor:
        hop = self.hop
        if jobs:
            wx = [self._x[w0 * hop - self._base:w1 * hop - self._base] for w0, w1, _, _ in jobs]
            outs = _run_encode_jobs(self.dac, wx, jobs, self.nq, self.rows_per_call)
            self.windows_run += len(jobs)
            self.frames_encoded += sum(w1 - w0 for w0, w1, _, _ in jobs)
            y = torch.cat([o[1] for o in outs], dim=1)
        else:
            y = torch.empty(self.nq, 0, dtype=torch.int64, device=self.dac.device)
        keep = self.planner.keep_from * hop          # only the samples the planner can still ask for stay
        if keep > self._base:
            self._x = self._x[keep - self._base:].clone()
            self._base = keep
        return y

    def push(self, samples) -> torch.Tensor:
        """-> the [nq, k] int64 codes that became final (on the codec's device; possibly k = 0)."""
        if self.planner.closed:
            raise RuntimeError("EncodeStream: push after flush")
        x = torch.as_tensor(samples)
        if x.ndim != 1 or x.dtype != torch.float32:
            raise TypeError(f"EncodeStream.push: samples must be 1-D float32 (got {x.dtype}, shape {tuple(x.shape)})")
        self._x = torch.cat([self._x, x.to(self.dac.device)])
        self.samples_received += int(x.numel())
        return self._run(self.planner.push(self.samples_received // self.hop - self.planner.received))

    def flush(self) -> torch.Tensor:
        """-> the codes of the rest of the stream; ends the session."""
        if self.planner.closed:
            raise RuntimeError("EncodeStream: flush after flush")
        jobs, part = [], self.samples_received % self.hop
        if part:                                      # the trailing partial frame, zero-padded as DAC.preprocess pads it
            self._x = torch.cat([self._x, torch.zeros(self.hop - part, dtype=torch.float32, device=self.dac.device)])
            jobs = self.planner.push(1)
        y = self._run(jobs + self.planner.flush())
        self._x = self._x[:0]
        return y


def encode_long(dac, audio, n_quantizers: Optional[int] = None, window_frames: int = 1024, rows_per_call: int = 4):
    """audio [1, 1, L] (L % hop == 0: `preprocess` pads) -> (z, codes, latents, None, None), bit for bit `dac.encode(audio, n_quantizers)`,
    through windows of at most `window_frames` frames, `rows_per_call` of them per ragged call, in ONE workspace sized for (rows_per_call,
    window_frames * hop) whatever L.  A recording that fits one window is one plain encode call."""
    if not isinstance(audio, torch.Tensor) or audio.ndim != 3 or audio.shape[0] != 1 or audio.shape[1] != 1:
        raise RuntimeError(f"encode_long expects [1, 1, L] audio (got {tuple(getattr(audio, 'shape', ()))})")
    if int(rows_per_call) < 1:
        raise ValueError(f"encode_long: rows_per_call must be >= 1 (got {rows_per_call})")
    hop, Lw = int(dac.hop_length), int(audio.shape[-1])
    if Lw % hop or Lw < hop:
        raise RuntimeError(f"encode_long: length {Lw} is not a positive multiple of the hop length {hop}; call preprocess() first")
    window_frames, rows_per_call, T = int(window_frames), int(rows_per_call), Lw // hop
    if T <= window_frames:
        return dac.encode(audio, n_quantizers)
    left, right = dac.encode_halo()
    if window_frames <= left + right:
        raise ValueError(f"encode_long: window_frames must exceed the encoder's halos {left} + {right} (got {window_frames})")
    x = audio.to(dac.device, torch.float32)[0, 0]
    planner = DecodePlanner(left, right, window_frames - left - right)
    jobs = planner.push(T) + planner.flush()
    ws = dac.encode_workspace(rows_per_call, window_frames * hop)
    z = codes = lat = None
    for g in range(0, len(jobs), rows_per_call):
        grp = jobs[g:g + rows_per_call]
        outs = _run_encode_jobs(dac, [x[w0 * hop:w1 * hop] for w0, w1, _, _ in grp], grp, n_quantizers, rows_per_call, ws=ws)
        for (_, _, e0, e1), (zj, cj, lj) in zip(grp, outs):
            if z is None:
                z = torch.empty(1, zj.shape[0], T, dtype=zj.dtype, device=zj.device)
                codes = torch.empty(1, cj.shape[0], T, dtype=cj.dtype, device=cj.device)
                lat = torch.empty(1, lj.shape[0], T, dtype=lj.dtype, device=lj.device)
            z[0, :, e0:e1], codes[0, :, e0:e1], lat[0, :, e0:e1] = zj, cj, lj
    return z, codes, lat, None, None
