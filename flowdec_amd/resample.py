"""Resampling on the device: torchaudio's polyphase sinc resampler as an exact HIP kernel, one-shot, ragged and streaming.

The filter bank is `audio.sinc_resample_kernel`'s array (the pinned restatement of torchaudio.functional.resample); the kernel
(csrc/resample.hip, include/flowdec_hip.h "Resampling") sums every output in float64 in ascending tap order and rounds once, so

  * `Resampler(o, n)(x)` is reproduced bit for bit by a plain NumPy loop (tests/resample_oracle.py), and differs from the host
    `audio.resample` by float32 rounding of the FIR only;
  * a clip's output does not depend on the batch it is in (`Resampler.batch`: one ragged call);
  * a stream's concatenated output (`ResampleStream`) is the one-shot output whatever the cut of the input into pushes.

`ResamplePlanner` is the host-only bookkeeping of a stream (no torch device): which outputs have become computable and which input
samples must be kept.  Before the end of the stream output m = q n + i is computable once its last tap q o + width + o - 1 has
arrived; `delay_samples` = width + o input samples.
"""
import ctypes as C
import math
from typing import List, NamedTuple, Optional, Tuple

import numpy as np
import torch

from . import _lib as L
from .audio import sinc_resample_kernel
from .batching import padded_rows

BANK_CAP = 1 << 24          # n * K coefficients (fd_resample_plan_create)


def rate_ratio(orig_freq: int, new_freq: int, lowpass_filter_width: int = 64, rolloff: float = 0.99) -> Tuple[int, int, int]:
    """-> (o, n, width) of `sinc_resample_kernel` without building the bank."""
    orig_freq, new_freq = int(orig_freq), int(new_freq)
    if orig_freq < 1 or new_freq < 1:
        raise ValueError(f"resample: rates must be positive (got {orig_freq} -> {new_freq})")
    g = math.gcd(orig_freq, new_freq)
    o, n = orig_freq // g, new_freq // g
    return o, n, math.ceil(lowpass_filter_width * o / (min(o, n) * rolloff))


def bank_fits(orig_freq: int, new_freq: int, lowpass_filter_width: int = 64, rolloff: float = 0.99) -> bool:
    """Whether the pair's filter bank is within the cap of the device resampler (equal rates need none)."""
    o, n, width = rate_ratio(orig_freq, new_freq, lowpass_filter_width, rolloff)
    return int(orig_freq) == int(new_freq) or n * (2 * width + o) <= BANK_CAP


class Released(NamedTuple):
    m0: int              # the outputs [m0, m0 + count) have become computable
    count: int
    retain_from: int     # input samples below this index are no longer needed


class ResamplePlanner:
    """Host bookkeeping of one resampled stream: `push(k)` / `flush()` -> Released."""

    def __init__(self, o: int, n: int, width: int):
        self.o, self.n, self.width = int(o), int(n), int(width)
        if self.o < 1 or self.n < 1 or self.width < 0:
            raise ValueError(f"ResamplePlanner: need o, n >= 1 and width >= 0 (got {o}, {n}, {width})")
        self.delay_samples = self.width + self.o
        self.received = self.released = 0
        self.ended = False

    def out_length(self, length: int) -> int:
        return -(-self.n * int(length) // self.o)

    @property
    def retain_from(self) -> int:
        """First input sample the next output reads (outputs are released by whole periods until the end)."""
        return max(0, (self.released // self.n) * self.o - self.width)

    def _release(self, upto: int) -> Released:
        m0, self.released = self.released, max(self.released, upto)
        return Released(m0, self.released - m0, self.retain_from)

    def push(self, k: int) -> Released:
        if self.ended:
            raise RuntimeError("ResamplePlanner: push after flush")
        if k < 0:
            raise ValueError(f"ResamplePlanner: push of {k} samples")
        self.received += int(k)
        periods = max(0, (self.received - self.width) // self.o)       # q is complete once q o + width + o - 1 < received
        return self._release(periods * self.n)

    def flush(self) -> Released:
        if self.ended:
            raise RuntimeError("ResamplePlanner: flush after flush")
        self.ended = True
        return self._release(self.out_length(self.received))


class Resampler:
    """torchaudio.functional.resample(x, orig_freq, new_freq, lowpass_filter_width, rolloff) on the device.

        r = Resampler(44100, 48000, device="cuda:0")
        y = r(x)                      # [..., L] float32 on the device -> [..., ceil(n L / o)]
        ys = r.batch([x0, x1, ...])   # 1-D clips of any lengths, ONE native call; each equals r(x_b) bit for bit

    Equal rates return the input unchanged.  A pair whose bank is over the cap (n K > 2^24) raises ValueError."""

    def __init__(self, orig_freq: int, new_freq: int, lowpass_filter_width: int = 64, rolloff: float = 0.99, device="cuda"):
        self.orig_freq, self.new_freq, self.lowpass_filter_width, self.rolloff = int(orig_freq), int(new_freq), int(lowpass_filter_width), float(rolloff)
        self.o, self.n, self.width = rate_ratio(orig_freq, new_freq, lowpass_filter_width, rolloff)
        self.K = 2 * self.width + self.o
        self.identity = self.orig_freq == self.new_freq
        self._plan = None
        if not self.identity and self.n * self.K > BANK_CAP:
            raise ValueError(f"Resampler: the filter bank of {self.orig_freq} -> {self.new_freq} Hz ({self.n} phases x {self.K} taps) is over the "
                             f"cap of 2^24 coefficients")
        self.device = torch.device(device)
        if self.identity:
            return
        self.device = L.cuda_device(self.device)
        if self.device.type != "cuda":
            raise RuntimeError("flowdec_amd: Resampler runs on the GPU (HIP is the only compute path)")
        bank, width, o, n = sinc_resample_kernel(self.orig_freq, self.new_freq, self.lowpass_filter_width, self.rolloff)
        assert (width, o, n) == (self.width, self.o, self.n) and bank.shape == (self.n, self.K) and bank.dtype == np.float32
        bank = np.ascontiguousarray(bank)
        plan = C.c_void_p()
        with torch.cuda.device(self.device):
            L.check(L.load().fd_resample_plan_create(bank.ctypes.data_as(C.c_void_p), self.o, self.n, self.width, C.byref(plan)))
        self._plan = plan

    def __del__(self):
        if getattr(self, "_plan", None):
            try:
                L.load().fd_resample_plan_destroy(self._plan)
            except Exception:
                pass
            self._plan = None

    def planner(self) -> ResamplePlanner:
        return ResamplePlanner(self.o, self.n, self.width)

    def out_length(self, length: int) -> int:
        if self.identity:
            return int(length)
        return int(L.load().fd_resample_out_length(int(length), self.o, self.n))

    def _check(self, x: torch.Tensor) -> None:
        if not x.is_cuda or x.device != self.device:
            raise RuntimeError(f"Resampler: the input lives on {x.device}, the plan on {self.device}")
        if x.dtype != torch.float32:
            raise TypeError(f"Resampler: float32 samples (got {x.dtype})")

    @torch.no_grad()
    def __call__(self, x: torch.Tensor) -> torch.Tensor:
        if self.identity:
            return x
        self._check(x)
        shape, length = x.shape, x.shape[-1]
        M = self.out_length(length)
        if x.numel() == 0:
            return x.new_empty(*shape[:-1], M)
        w = x.reshape(-1, length).contiguous()
        y = torch.empty(w.shape[0], M, dtype=torch.float32, device=self.device)
        lib = L.load()
        with torch.cuda.device(self.device):
            for b0 in range(0, w.shape[0], 65535):
                b1 = min(b0 + 65535, w.shape[0])
                L.check(lib.fd_resample(self._plan, L.ptr(w[b0:b1]), None, b1 - b0, length, L.ptr(y[b0:b1]), M, L.stream()))
        return y.reshape(*shape[:-1], M)

    @torch.no_grad()
    def batch(self, clips: List[torch.Tensor]) -> List[torch.Tensor]:
        if self.identity:
            return list(clips)
        for c in clips:
            self._check(c)
            if c.dim() != 1:
                raise ValueError("Resampler.batch: 1-D clips")
        if not clips:
            return []
        if len(clips) > 65535:
            raise ValueError("Resampler.batch: at most 65535 clips per call")
        lens = [int(c.numel()) for c in clips]
        Lmax = max(max(lens), 1)
        Mmax = self.out_length(Lmax)
        x, lengths = padded_rows(clips, Lmax, self.device)
        y = torch.empty(len(clips), Mmax, dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            L.check(L.load().fd_resample(self._plan, L.ptr(x), L.ptr(lengths), len(clips), Lmax, L.ptr(y), Mmax, L.stream()))
        return [y[b, :self.out_length(n)].clone() for b, n in enumerate(lens)]

    @torch.no_grad()
    def span(self, x: Optional[torch.Tensor], x0: int, total: int, m0: int, count: int) -> torch.Tensor:
        """fd_resample_span: the outputs [m0, m0 + count) of a recording of `total` samples (-1: unknown) of which `x` holds
        [x0, x0 + len(x))."""
        y = torch.empty(int(count), dtype=torch.float32, device=self.device)
        nx = 0 if x is None else int(x.numel())
        if nx:
            self._check(x)
            x = x.contiguous()
        with torch.cuda.device(self.device):
            L.check(L.load().fd_resample_span(self._plan, L.ptr(x) if nx else None, int(x0), nx, int(total), int(m0), int(count), L.ptr(y), L.stream()))
        return y


def get_resampler(orig_freq: int, new_freq: int, lowpass_filter_width: int = 64, rolloff: float = 0.99, device="cuda") -> Resampler:
    """The cached `Resampler` of (o, n, lowpass_filter_width, rolloff, device)."""
    dev = L.cuda_device(device)
    o, n, _ = rate_ratio(orig_freq, new_freq, lowpass_filter_width, rolloff)     # (o, n): the bank depends on the ratio only
    return L.cached_plan(dev, ("resample", o, n, int(lowpass_filter_width), float(rolloff)), lambda: Resampler(o, n, lowpass_filter_width, rolloff, dev),
                         enter=False)      # (a Resampler enters its own device; equal rates need none, and "cpu" is allowed for them)


def resample_device(y: torch.Tensor, sr: int, target: int, lowpass_filter_width: int = 64, rolloff: float = 0.99) -> torch.Tensor:
    """`audio.resample` on the device `y` lives on: [..., L] float32 -> [..., ceil(n L / o)], plans cached per
    (o, n, lowpass_filter_width, rolloff, device)."""
    if int(sr) == int(target):
        return y
    if not y.is_cuda:
        raise RuntimeError("flowdec_amd: resample_device takes a tensor on the GPU (HIP is the only compute path)")
    return get_resampler(sr, target, lowpass_filter_width, rolloff, y.device)(y.float())


class ResampleStream:
    """A stateful resampler: `push(block)` -> the outputs that became computable (a float32 tensor on the device, often empty),
    `flush()` -> the rest.  Blocks are float32 or int16 PCM (x * 2^-15, exact), tensors or arrays of any size, on the CPU or the
    device.  Concatenated, the output is `resampler(all input)` bit for bit however the input was cut."""

    def __init__(self, resampler: Resampler):
        self.r = resampler
        self.dev = resampler.device
        self.planner = resampler.planner()
        self.delay_samples = 0 if resampler.identity else self.planner.delay_samples
        self._carry = None            # device float32: the samples [_carry0, received)
        self._carry0 = 0

    def _block(self, x) -> torch.Tensor:
        x = torch.as_tensor(x).reshape(-1)
        if x.is_cuda and x.device != self.dev:
            raise RuntimeError(f"ResampleStream.push: the block lives on {x.device}, the resampler on {self.dev}")
        if x.dtype == torch.int16:
            return x.to(self.dev).to(torch.float32) * (1.0 / 32768.0)
        if x.dtype != torch.float32:
            raise TypeError(f"ResampleStream.push: float32 or int16 samples (got {x.dtype})")
        return x.to(self.dev)

    @torch.no_grad()
    def push(self, x) -> torch.Tensor:
        x = self._block(x)
        if self.r.identity:
            self.planner.push(x.numel())
            return x.clone()
        rel = self.planner.push(x.numel())
        buf = x if self._carry is None or self._carry.numel() == 0 else (torch.cat([self._carry, x]) if x.numel() else self._carry)
        return self._advance(buf, rel, -1)

    @torch.no_grad()
    def flush(self) -> torch.Tensor:
        rel = self.planner.flush()
        if self.r.identity:
            return torch.empty(0, dtype=torch.float32, device=self.dev)
        buf = self._carry if self._carry is not None else torch.empty(0, dtype=torch.float32, device=self.dev)
        return self._advance(buf, rel, self.planner.received)

    def _advance(self, buf: torch.Tensor, rel: Released, total: int) -> torch.Tensor:
        y = self.r.span(buf, self._carry0, total, rel.m0, rel.count) if rel.count else torch.empty(0, dtype=torch.float32, device=self.dev)
        keep = rel.retain_from - self._carry0                  # >= 0: retain_from never goes back
        if keep > 0 or buf is not self._carry:
            self._carry = buf[keep:].clone()                   # (a copy: `buf` may be the caller's own block)
            self._carry0 = rel.retain_from
        return y
