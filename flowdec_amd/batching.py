"""How clips of different lengths become native calls: the two batch plans of the package and the one staging function.

* T_pad buckets (`padded_frames_of`, `plan_clip_batches`, `_ragged_bucket`): the model's calls take clips whose spectrograms pad to ONE
  frame count -- enhance_cli, dist.sharded_enhance_batch and loss.valid_loss_batch plan with these.
* Length-sorted batches (`length_sorted_batches`): the metric and resampler kernels take rows of any lengths, so similar lengths share a
  call and little of a row is padding.
* `padded_rows`: clips -> zero-padded rows [B, Lrow] on the device with their int32 lengths, for every ragged call.

Imports `_lib` and `ops` only.
"""
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
