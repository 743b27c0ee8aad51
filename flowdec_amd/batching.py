"""How clips of different lengths become native calls: the two batch plans of the package and the one staging function.

* T_pad buckets (`padded_frames_of`, `plan_clip_batches`, `_ragged_bucket`): the model's calls take clips whose spectrograms pad to ONE
  frame count -- enhance_cli, dist.sharded_enhance_batch and loss.valid_loss_batch plan with these.
* Length-sorted batches (`length_sorted_batches`): the metric and resampler kernels take rows of any lengths, so similar lengths share a
  call and little of a row is padding.
* `padded_rows`: clips -> zero-padded rows [B, Lrow] on the device with their int32 lengths, for every ragged call.
* `as_clips`, `ragged_batches`: the ONE loop over length-sorted batches that every measurement (metrics, specdist, segsnr, loudness,
  align) makes its native calls from.

Imports `_lib` and `ops` only.
"""
import contextlib
from typing import List, Sequence, Tuple

import torch

from . import _lib as L
from . import ops


def padded_frames_of(num_samples: int, hop: int = 384) -> int:
    """T_pad of a clip of `num_samples` samples: pad_spec(1 + L // hop) (util/other.py:25-52) -- the bucket key of `enhance_batch`."""
    lib = L.load()
    return int(lib.fd_padded_frames(lib.fd_num_frames(int(num_samples), int(hop))))


def _ragged_bucket(clips, cfg):
    """The bucket rule of every `enhance_batch`: clips [L], [1, L] or [1, 1, L] that all pad to ONE frame count.  -> (the clips flattened,
    their lengths, T_pad, the row length).  The row length is the bucket's LARGEST possible clip (1 + Lrow // hop == T_pad): one
    workspace / one hipGraph per (B, T_pad)."""
    lib = L.load()
    hop = cfg["hop"]
    flat = []
    for i, c in enumerate(clips):
        if c.ndim > 3 or any(d != 1 for d in c.shape[:-1]):
            raise RuntimeError(f"enhance_batch: clip {i} must be [L], [1, L] or [1, 1, L] (got {tuple(c.shape)})")
        flat.append(c.reshape(-1))
    lens = [int(c.numel()) for c in flat]
    Tps = {lib.fd_padded_frames(lib.fd_num_frames(l, hop)) for l in lens}
    if len(Tps) != 1:
        raise RuntimeError(f"enhance_batch: the clips pad to different frame counts {sorted(Tps)}; one call takes one T_pad bucket "
                           f"(bucket with flowdec_amd.model.padded_frames_of)")
    Tp = Tps.pop()
    Lrow = hop * Tp - 1
    ops.check_ragged_lengths(lens, Lrow, cfg["n_fft"], hop)
    return flat, lens, Tp, Lrow


def _to_3d(y, who, rows="B"):
    """[L] / [1, L] / [B, 1, L] -> ([B, 1, L], the number of axes added in front: `squeeze_dims`, model.py:146-149), or raise."""
    y3, squeeze_dims = y, 0
    while y3.ndim < 3:
        y3 = y3.unsqueeze(0); squeeze_dims += 1
    if y3.ndim != 3 or y3.shape[1] != 1:
        raise RuntimeError(f"{who} [L], [1, L] or [{rows}, 1, L] waveforms (got {tuple(y.shape)})")
    return y3, squeeze_dims


def plan_clip_batches(lengths: Sequence[int], hop: int, batch_clips: int) -> List[Tuple[int, List[int]]]:
    """Clips of `lengths` samples bucketed by the frame count their spectrogram pads to (`padded_frames_of`), buckets in ascending
    T_pad, every bucket cut in clip order into batches of at most `batch_clips`.  -> [(T_pad, clip indices)], the same on every rank."""
    batch_clips = max(int(batch_clips), 1)
    buckets = {}
    for i, n in enumerate(lengths):
        buckets.setdefault(padded_frames_of(int(n), hop), []).append(i)
    return [(tp, buckets[tp][k:k + batch_clips]) for tp in sorted(buckets) for k in range(0, len(buckets[tp]), batch_clips)]


def length_sorted_batches(lengths, batch: int):
    """Indices sorted by length (ties by index) and cut into batches of at most `batch`: the clips of one call have similar lengths, so
    little of a row is padding.  The results do not depend on this (a clip's bits are the same in any batch)."""
    order = sorted(range(len(lengths)), key=lambda i: (lengths[i], i))
    batch = max(int(batch), 1)
    return [order[i:i + batch] for i in range(0, len(order), batch)]


@torch.no_grad()
def padded_rows(clips, Lrow: int, device, out=None):
    """1-D clips -> (rows float32 [B, Lrow] on `device`, zero behind each clip; lens int32 [B] on `device`).  Host clips are staged in
    ONE host block and copied once; if any clip already lives on a GPU (a device resampler left it there) the clips go into the device
    buffer one by one, with no host round trip.  out: a caller-owned float32 [B, Lrow] buffer to fill instead (`device` is then its
    device); every element of it is written."""
    lens = [int(c.numel()) for c in clips]
    for b, c in enumerate(clips):
        if c.dim() != 1:
            raise ValueError(f"padded_rows: 1-D clips (clip {b} is {tuple(c.shape)})")
        if lens[b] > Lrow:
            raise ValueError(f"padded_rows: clip {b} has {lens[b]} samples, a row holds {Lrow}")
    if out is not None and (out.shape != (len(lens), Lrow) or out.dtype != torch.float32):
        raise ValueError(f"padded_rows: out must be float32 [{len(lens)}, {Lrow}] (got {out.dtype} {tuple(out.shape)})")
    dev = torch.device(device) if out is None else out.device
    if dev.type != "cuda" or any(c.is_cuda for c in clips):
        rows = torch.zeros(len(lens), Lrow, dtype=torch.float32, device=dev) if out is None else out.zero_()
        for b, c in enumerate(clips):
            rows[b, :lens[b]].copy_(c)
    else:
        block = torch.zeros(len(lens), Lrow, dtype=torch.float32)
        for b, c in enumerate(clips):
            block[b, :lens[b]].copy_(c)
        rows = block.to(dev) if out is None else out.copy_(block)
    return rows, torch.tensor(lens, dtype=torch.int32).to(dev)


def as_clips(*lists):
    """The signals of every list as 1-D tensors: one entry per clip in each list, the signals of one clip equally long and not empty."""
    out = [[torch.as_tensor(c).reshape(-1) for c in l] for l in lists]
    n = len(out[0])
    for l in out[1:]:
        if len(l) != n:
            raise ValueError("metrics: the lists must have one entry per clip each")
    for i in range(n):
        if len({int(l[i].numel()) for l in out}) != 1:
            raise ValueError(f"metrics: the signals of clip {i} differ in length ({[int(l[i].numel()) for l in out]})")
        if out[0][i].numel() < 1:
            raise ValueError(f"metrics: clip {i} is empty")
    return out


def ragged_batches(lists, batch, device, call, outs, own_rows: bool = False, host_call: bool = False):
    """The loop of every measurement's batch function: the clips of `lists` (one list of 1-D tensors per signal) in length-sorted batches
    of `batch` as zero-padded rows on `device`; call(rows, lens, idx, Lrow) makes the native call for the clips `idx` and returns one
    sequence per entry of `outs`, whose k-th item lands in outs[.][idx[k]] (an array or a list).  What belongs to single clips (a lag, a
    window) `call` builds from `idx`.
    The signals of a clip are equally long (`as_clips`): rows = one [B, Lrow] tensor per list, lens = their int32 [B] lengths, Lrow = the
    batch's longest clip.  own_rows: the signals of a clip may differ in length, even be empty; clips are sorted by their longest signal and
    every list is staged at its OWN row length, at least 1: lens and Lrow are then lists, one entry per list.
    A device that is not a GPU is refused by torch.cuda.device before anything is staged: `call` hands the rows to a kernel.  host_call:
    `call` runs on the host (a test's stand-in); device "cpu" then stages on the host and torch.cuda is never touched."""
    dev = L.cuda_device(device)
    lengths = [[int(c.numel()) for c in l] for l in lists]
    with contextlib.nullcontext() if host_call and dev.type != "cuda" else torch.cuda.device(dev):
        for idx in length_sorted_batches([max(ls) for ls in zip(*lengths)], batch):
            Lrows = [max(max(ls[i] for i in idx), 1) for ls in lengths]
            staged = [padded_rows([l[i] for i in idx], Lrow, dev) for l, Lrow in zip(lists, Lrows)]
            rows, lens = [r for r, _ in staged], [n for _, n in staged]
            for out, got in zip(outs, call(rows, lens, idx, Lrows) if own_rows else call(rows, lens[0], idx, Lrows[0])):
                for k, i in enumerate(idx):
                    out[i] = got[k]
