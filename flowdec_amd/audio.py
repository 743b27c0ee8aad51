"""File lists, wav files and the host resampler: what every command line and script of the package reads its audio with.

* `read_list` / `split_pair` -- the list formats of the reference's enhance.py (:146-164).
* `load_wav` / `wav_info` / `save_wav` -- wav I/O in torchaudio's conventions (float32 [C, L] in [-1, 1]).
* `sinc_resample_kernel` / `resample` -- the pinned restatement of torchaudio.functional.resample(..., lowpass_filter_width=64)
  (enhance.py:118; torchaudio itself is not a dependency).  The bank is also what the device resampler (flowdec_amd/resample.py) runs.
* `resample_to` -- the one router between the host resampler and the device one (`--resample host|device` of the command lines).
* `load_mono` -- the reference's load48000 (util/other.py:137-).

Imports nothing of the package but, inside `resample_to`, the device resampler.
"""
import math
import sys
from dataclasses import dataclass, field
from typing import List, Optional, Tuple

import numpy as np
import torch


# ------------------------------------------------------------------------------------------------
# file lists / wav I/O
# ------------------------------------------------------------------------------------------------
@dataclass
class FileList:
    """A parsed `--files` list: the inputs to enhance and, for pair lists, the clean reference each one belongs to."""
    inputs: List[str] = field(default_factory=list)
    clean: Optional[List[str]] = None     # None for a plain list

    @property
    def from_pairs(self) -> bool:
        return self.clean is not None


def split_pair(entry: str) -> List[str]:
    """`clean ---> coded` if the arrow is present, else `clean,coded` if a comma is (the reference's precedence, enhance.py:153-158:
    a path with commas in an arrow line is not cut at the comma)."""
    if " ---> " in entry:
        return entry.split(" ---> ")
    if "," in entry:
        return entry.split(",")
    return [entry]


def read_list(listfile: str) -> FileList:
    """The list formats of the reference (enhance.py:146-164): one path per line, or pair lines `clean ---> coded` /
    `clean,coded` of which the SECOND entry is the file to enhance; further fields are ignored like there (the tool's own
    `triples_list` output `clean ---> noisy ---> out` can be fed back in), with a warning.  A plain line after a pair line is an
    error there (an assert); here it is a ValueError naming the line."""
    out = FileList()
    with open(listfile, "r") as f:
        for lineno, raw in enumerate(f, 1):
            entry = raw.strip()
            if not entry:
                continue
            parts = split_pair(entry)
            if len(parts) > 2:
                print(f"warning: {listfile}:{lineno}: {len(parts)} fields in a pair line, using the first two (clean, coded)", file=sys.stderr)
            if len(parts) >= 2:
                if out.clean is None:
                    if out.inputs:
                        raise ValueError(f"{listfile}:{lineno}: pair line after plain paths -- inconsistent file list format")
                    out.clean = []
                out.clean.append(parts[0]); out.inputs.append(parts[1])
            elif out.from_pairs:
                raise ValueError(f"{listfile}:{lineno}: plain path after pair lines -- inconsistent file list format")
            else:
                out.inputs.append(entry)
    return out


def load_wav(path: str) -> Tuple[torch.Tensor, int]:
    """-> (float32 tensor [C, L] in [-1, 1], sampling rate), like torchaudio.load."""
    from scipy.io import wavfile
    sr, data = wavfile.read(path)
    if data.dtype == np.int16:
        x = data.astype(np.float32) / 32768.0
    elif data.dtype == np.int32:
        x = data.astype(np.float32) / 2147483648.0
    elif data.dtype == np.uint8:
        x = (data.astype(np.float32) - 128.0) / 128.0
    else:
        x = data.astype(np.float32)
    if x.ndim == 1:
        x = x[:, None]
    return torch.from_numpy(np.ascontiguousarray(x.T)), int(sr)


def wav_info(path: str) -> Tuple[int, int, int]:
    """-> (samples per channel, sampling rate, channels) from the header only (memory-mapped: the data is not read)."""
    from scipy.io import wavfile
    sr, data = wavfile.read(path, mmap=True)
    return int(data.shape[0]), int(sr), (1 if data.ndim == 1 else int(data.shape[1]))


def resampled_length(length: int, sr: int, target: int) -> int:
    """Samples `resample` returns for `length` input samples: ceil(n * L / o) with o, n = sr, target over their gcd."""
    if int(sr) == int(target):
        return int(length)
    g = math.gcd(int(sr), int(target))
    return int(math.ceil((int(target) // g) * length / (int(sr) // g)))


def save_wav(path: str, x: torch.Tensor, sr: int) -> None:
    """float32 wav, [C, L] or [L] (the reference saves float tensors through torchaudio.save)."""
    from scipy.io import wavfile
    a = x.detach().cpu().float().numpy()
    if a.ndim == 2:
        a = a.T
    wavfile.write(path, sr, np.ascontiguousarray(a, dtype=np.float32))


# ------------------------------------------------------------------------------------------------
# resampling
# ------------------------------------------------------------------------------------------------
def sinc_resample_kernel(orig_freq: int, new_freq: int, lowpass_filter_width: int = 64, rolloff: float = 0.99):
    """The polyphase filter bank of torchaudio.functional.resample (resampling_method='sinc_interp_hann', the default), restated
    from its published definition: with o = orig/gcd, n = new/gcd, f = min(o, n) * rolloff and width = ceil(lpw * o / f),
    phase i in [0, n) and tap k in [-width, width + o):
        t = clamp((k / o - i / n) * f, -lpw, lpw);   h[i, k] = sinc(t) * cos^2(pi * t / (2 * lpw)) * f / o      (sinc(t) = sin(pi t)/(pi t))
    Returns (kernel [n, 2 * width + o] float32 computed in float64 like torchaudio, width, o, n)."""
    g = math.gcd(int(orig_freq), int(new_freq))
    o, n = int(orig_freq) // g, int(new_freq) // g
    f = min(o, n) * rolloff
    width = math.ceil(lowpass_filter_width * o / f)
    k = np.arange(-width, width + o, dtype=np.float64)[None, :] / o
    i = np.arange(0, -n, -1, dtype=np.float64)[:, None] / n
    t = np.clip((i + k) * f, -lowpass_filter_width, lowpass_filter_width)
    window = np.cos(t * math.pi / lowpass_filter_width / 2) ** 2
    tp = t * math.pi
    with np.errstate(invalid="ignore", divide="ignore"):
        sinc = np.where(tp == 0, 1.0, np.sin(tp) / tp)
    return (sinc * window * (f / o)).astype(np.float32), width, o, n


def resample(y: torch.Tensor, sr: int, target: int, lowpass_filter_width: int = 64, rolloff: float = 0.99) -> torch.Tensor:
    """torchaudio.functional.resample(y, sr, target, lowpass_filter_width=64) as the reference calls it (enhance.py:118):
    zero-pad by (width, width + o), correlate with the n-phase filter bank at stride o, interleave the phases, keep
    ceil(n * L / o) samples.  Host-side float32 (file pre-processing, not on the hot path)."""
    if int(sr) == int(target):
        return y
    kern, width, o, n = sinc_resample_kernel(sr, target, lowpass_filter_width, rolloff)
    shape = y.shape
    w = y.reshape(-1, shape[-1]).float()
    length = w.shape[-1]
    w = torch.nn.functional.pad(w, (width, width + o))
    r = torch.nn.functional.conv1d(w[:, None], torch.from_numpy(kern)[:, None], stride=o)       # [num, n, frames]
    r = r.transpose(1, 2).reshape(w.shape[0], -1)[:, : int(math.ceil(n * length / o))]
    return r.reshape(*shape[:-1], r.shape[-1])


RESAMPLE_HELP = ("where a file that is not at --sr is resampled.  host: on the CPU (the default).  device: the same polyphase filter as a HIP "
                 "kernel on the current GPU (flowdec_amd.resample), summed in float64 and rounded once -- the values differ from host mode by "
                 "float32 rounding of the FIR.  A rate pair over the device resampler's bank cap falls back to the host path, with one printed line")


def resample_to(y: torch.Tensor, sr: int, target: int, mode: str = "host", device=None, lowpass_filter_width: int = 64) -> torch.Tensor:
    """`--resample`: y [..., L] at `sr` -> at `target`.  mode='host': `resample` on the CPU; 'device': the same filter on `device`
    (flowdec_amd.resample; the result stays there).  A rate pair over the bank cap of the device resampler takes the host path, with
    one printed line."""
    if mode not in ("host", "device"):
        raise ValueError(f"resample_to: mode is 'host' or 'device' (got {mode!r})")
    if mode == "device":
        from . import resample as fd_resample     # lazy: resample.py takes the filter bank from this module at its top
        if fd_resample.bank_fits(sr, target, lowpass_filter_width):
            return fd_resample.resample_device(y.to(device), sr, target, lowpass_filter_width=lowpass_filter_width)
        print(f"--resample device: the filter bank of {sr} -> {target} Hz is over the device resampler's cap; resampling on the host")
    return resample(y, sr, target, lowpass_filter_width=lowpass_filter_width)


def load_mono(path: str, sr: int, resample: str = "host") -> torch.Tensor:
    """load48000 (util/other.py:137-) for the rate `sr`: -> 1-D float32 tensor, the mean of the channels, resampled when the rate differs
    (lowpass_filter_width=256): resample='host' on the CPU, 'device' on the current GPU (the signal then stays there)."""
    au, fs = load_wav(path)
    if au.shape[0] != 1:
        au = au.mean(dim=0, keepdim=True)
    if fs != sr:
        au = resample_to(au, fs, sr, mode=resample, device="cuda", lowpass_filter_width=256)
    return au[0].contiguous()
