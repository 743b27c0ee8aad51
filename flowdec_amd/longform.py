"""Long-form planner: a recording of any length as overlapping rows of ONE (B, T_pad) bucket (pure host code, no GPU, no torch).

A row is a stretch of the recording that starts on the recording's frame grid (a multiple of `hop`), so that its STFT frames are the
recording's frames and the seeded noise can be addressed by the ABSOLUTE frame (`frame0 = start / hop`, include/flowdec_hip.h
"Long-form"): two rows that overlap start from bit-identical noise in their overlap.  Neighbouring rows overlap by two halos; each keeps
what lies between its boundaries, and `xfade` samples centred on a boundary are a raised-cosine cross-fade of the two rows.

Geometry (W = row_frames * hop - 1 samples = the longest clip that still has row_frames frames, the bucket rule of `enhance_batch`):

  * row j of all but the last starts at j * (row_frames - 2 * halo_frames - 1) * hop and is W samples long;
  * the last row ends at n: its start is n - W rounded UP to a multiple of hop (so it is W - hop < length <= W samples long and pads to
    row_frames frames like the others -- one bucket, one workspace, one graph);
  * the boundary between the rows j - 1 and j lies (row_frames - halo_frames - 1) * hop after the start of row j - 1: as late as the
    earlier row allows.  The earlier row then has halo_frames * hop + hop - 1 samples beyond it; the later row starts halo_frames * hop
    before it, or earlier (the shifted last row).

The stride is one frame shorter than row_frames - 2 * halo_frames because a row of row_frames FRAMES is one sample short of
row_frames * hop SAMPLES: without it the earlier row would have halo_frames * hop - 1 samples beyond the boundary.
"""
from typing import List, NamedTuple, Optional, Tuple

import numpy as np


class Row(NamedTuple):
    start: int                 # first sample of the row in the recording (a multiple of hop)
    length: int                # samples of the row (<= W)
    frame0: int                # start / hop: the absolute frame of the row's first STFT frame
    keep: Tuple[int, int]      # [lo, hi): the samples of the recording this row owns (the kept ranges partition [0, n))
    xfade_lo: Optional[int]    # centre of the cross-fade with the previous row (= keep[0]), None for the first row
    xfade_hi: Optional[int]    # centre of the cross-fade with the next row (= keep[1]), None for the last row


def row_samples(row_frames: int, hop: int) -> int:
    """W: the longest row that still has `row_frames` frames (1 + W // hop == row_frames)."""
    return int(row_frames) * int(hop) - 1


def plan_rows(n_samples: int, hop: int, row_frames: int = 3712, halo_frames: int = 256, xfade: Optional[int] = None) -> List[Row]:
    """The rows of a recording of `n_samples` samples (module docstring).  xfade=None: 2 * hop."""
    n, hop, rf, halo = int(n_samples), int(hop), int(row_frames), int(halo_frames)
    xfade = 2 * hop if xfade is None else int(xfade)
    if n < 1 or hop < 1:
        raise ValueError(f"plan_rows: need n_samples >= 1 and hop >= 1 (got {n}, {hop})")
    if rf < 64 or rf % 64:
        raise ValueError(f"plan_rows: row_frames must be a positive multiple of 64 (got {rf})")
    if halo < 0 or xfade < 0 or xfade % 2:
        raise ValueError(f"plan_rows: halo_frames must be >= 0 and xfade even and >= 0 (got {halo}, {xfade})")
    if xfade // 2 > halo * hop:
        raise ValueError(f"plan_rows: half the cross-fade ({xfade // 2} samples) must lie inside the halo ({halo * hop} samples)")
    W = row_samples(rf, hop)
    if n <= W:
        return [Row(0, n, 0, (0, n), None, None)]
    stride = (rf - 2 * halo - 1) * hop
    if stride < max(xfade, hop):
        raise ValueError(f"plan_rows: row_frames {rf} leaves no room between two halos of {halo} frames and a cross-fade of {xfade} samples")
    starts = [0]
    while starts[-1] + W < n:
        starts.append(starts[-1] + stride)
    starts[-1] = -(-(n - W) // hop) * hop          # the last row ends at n; its start rounded up onto the frame grid
    bounds = [s + (rf - halo - 1) * hop for s in starts[:-1]]
    rows = []
    for j, s in enumerate(starts):
        lo = 0 if j == 0 else bounds[j - 1]
        hi = n if j == len(starts) - 1 else bounds[j]
        rows.append(Row(s, min(W, n - s), s // hop, (lo, hi), None if j == 0 else lo, None if j == len(starts) - 1 else hi))
    return rows


def stitch_weights(xfade: int) -> np.ndarray:
    """The cross-fade table fd_stitch_chunks reads: w_i = 0.5 - 0.5 cos(pi (i + 0.5) / xfade), i < xfade, evaluated in float64 and rounded
    once to float32.  The weight of the LATER row; the earlier row's is 1 - w in exact arithmetic (out = a + w (b - a))."""
    i = np.arange(int(xfade), dtype=np.float64)
    return (0.5 - 0.5 * np.cos(np.pi * (i + 0.5) / max(int(xfade), 1))).astype(np.float32)


def stitch_reference(row_outputs, rows: List[Row], xfade: int) -> np.ndarray:
    """NumPy float32 restatement of fd_stitch_chunks (each of a + w * (b - a)'s three operations rounded on its own): the recording's
    output from its rows' outputs (row_outputs[j][k] = sample rows[j].start + k)."""
    n = rows[-1].keep[1]
    out = np.empty(n, dtype=np.float32)
    for r, o in zip(rows, row_outputs):
        lo, hi = r.keep
        out[lo:hi] = np.asarray(o, dtype=np.float32)[lo - r.start:hi - r.start]
    w, half = stitch_weights(xfade), int(xfade) // 2
    for j in range(1, len(rows)):
        c = rows[j].xfade_lo
        a = np.asarray(row_outputs[j - 1], dtype=np.float32)[c - half - rows[j - 1].start:c + half - rows[j - 1].start]
        b = np.asarray(row_outputs[j], dtype=np.float32)[c - half - rows[j].start:c + half - rows[j].start]
        d = (b - a).astype(np.float32)
        out[c - half:c + half] = (a + (w * d).astype(np.float32)).astype(np.float32)
    return out


def chunk_row_frames(chunk_seconds: float, sampling_rate: int, hop: int) -> int:
    """`--chunk-seconds S` -> row_frames: the frames of S seconds rounded DOWN to a multiple of 64, at least 64."""
    frames = int(float(chunk_seconds) * int(sampling_rate)) // int(hop)
    return max(64, frames // 64 * 64)


def chunk_halo_frames(row_frames: int, halo_frames: int = 256) -> int:
    """The halo the command line uses with rows of `row_frames`: the default, but never more than a quarter of the row (rows shorter than
    1024 frames would otherwise be mostly, or entirely, halo)."""
    return min(int(halo_frames), int(row_frames) // 4)


class StreamRow(NamedTuple):
    row: Row                   # the row, field for field what plan_rows gives for the finished recording
    finished: Tuple[int, int]  # [lo, hi): the samples of the recording that are final once this row has run (consecutive, from 0)
    index: int                 # the row's number in the recording
    last: bool


class StreamPlanner:
    """`plan_rows` for a recording whose length is not known yet: fed a running sample count (`push`) and one final `flush`, it yields the
    rows of `plan_rows(n, ...)` -- the same fields -- as soon as each can run.

    With h = hop, W = row_frames * h - 1, S = (row_frames - 2 * halo_frames - 1) * h, Bo = (row_frames - halo_frames - 1) * h,
    half = xfade / 2:

      * regular row j = [j * S, j * S + W) is READY as soon as more than j * S + W samples have arrived: plan_rows shifts only the last
        row, and a row that has a sample beyond its end is not the last;
      * `flush()` at n samples yields the last row as plan_rows places it: (0, n) if n <= W, else start ceil((n - W) / h) * h;
      * after regular row j the samples [lo_j - half, hi_j - half) are final (lo_j = (j - 1) * S + Bo, hi_j = j * S + Bo; lo_0 - half
        reads 0): the cross-fade around hi_j needs the next row.  After the last row they run to n;
      * RETENTION INVARIANT: with j the next regular row, every row still to come -- regular or last -- starts at or after
        `retain_from` = (j - 1) * S (0 for j = 0), the start of the previous regular row.  (The last row ends at n with
        (j - 1) * S + W < n <= j * S + W, so it starts in ((j - 1) * S, j * S]: up to S - h before the next regular start.)  A session
        therefore keeps its input from `retain_from` on, and `ring_samples` = S + W is enough to hold any row that can come next;
      * worst-case algorithmic delay: sample hi_{j-1} - half becomes final with row j, i.e. once j * S + W + 1 samples have arrived --
        `delay_samples` = (row_frames - halo_frames) * h + half samples of FURTHER input (plus the row's compute time);
      * `push` refuses input once n / h + t_pad would reach 2^31 absolute frames (the noise contract, include/flowdec_hip.h).
    """

    def __init__(self, hop: int, row_frames: int = 3712, halo_frames: int = 256, xfade: Optional[int] = None, t_pad: Optional[int] = None):
        self.hop, self.rf, self.halo = int(hop), int(row_frames), int(halo_frames)
        self.xfade = 2 * self.hop if xfade is None else int(xfade)
        self.W = row_samples(self.rf, self.hop)
        plan_rows(self.W + 1, self.hop, self.rf, self.halo, self.xfade)      # the argument checks of plan_rows, incl. "no room between two halos"
        self.S = (self.rf - 2 * self.halo - 1) * self.hop
        self.Bo = (self.rf - self.halo - 1) * self.hop
        self.half = self.xfade // 2
        self.t_pad = self.rf if t_pad is None else int(t_pad)
        self.delay_samples = (self.rf - self.halo) * self.hop + self.half
        self.ring_samples = self.S + self.W
        self.n = 0                 # samples arrived
        self.j = 0                 # the next regular row
        self.done = 0              # samples final so far: the next finished range starts here
        self.closed = False

    @property
    def retain_from(self) -> int:
        """The first sample a session still needs (the retention invariant of the class docstring)."""
        return max(self.j - 1, 0) * self.S

    def push(self, count: int) -> None:
        count = int(count)
        if self.closed or count < 0:
            raise ValueError("StreamPlanner.push: the stream is flushed" if self.closed else f"StreamPlanner.push: negative count {count}")
        if (self.n + count) // self.hop + self.t_pad >= 2 ** 31:
            raise RuntimeError(f"StreamPlanner.push: {self.n + count} samples exceed the 2^31 absolute frames of the noise contract")
        self.n += count

    def ready(self) -> bool:
        return not self.closed and self.n > self.j * self.S + self.W

    def next_row(self) -> Optional[StreamRow]:
        """The next regular row if it is ready, else None."""
        if not self.ready():
            return None
        j, s = self.j, self.j * self.S
        lo, hi = (0 if j == 0 else s - self.S + self.Bo), s + self.Bo
        out = StreamRow(Row(s, self.W, s // self.hop, (lo, hi), None if j == 0 else lo, hi), (self.done, hi - self.half), j, False)
        assert out.finished[0] == max(lo - self.half, 0) and s >= self.retain_from
        self.j, self.done = j + 1, hi - self.half
        return out

    def flush(self) -> StreamRow:
        """The last row.  Call it once every ready regular row has been taken (`next_row()` is None)."""
        if self.closed or self.ready() or self.n < 1:
            raise ValueError("StreamPlanner.flush: " + ("already flushed" if self.closed else "regular rows are still ready" if self.n else "no input"))
        self.closed = True
        n, j = self.n, self.j
        if j == 0:                                                # n <= W: the recording is one row
            out = StreamRow(Row(0, n, 0, (0, n), None, None), (0, n), 0, True)
        else:
            s = -(-(n - self.W) // self.hop) * self.hop           # as plan_rows: n - W rounded UP onto the frame grid
            lo = (j - 1) * self.S + self.Bo
            out = StreamRow(Row(s, n - s, s // self.hop, (lo, n), lo, None), (self.done, n), j, True)
            assert s >= self.retain_from + self.hop and out.finished[0] == lo - self.half
        self.done = n
        return out
