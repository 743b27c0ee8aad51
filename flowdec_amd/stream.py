"""Streaming enhance: push / flush sessions whose output is, bit for bit, the model's long-form enhance (`FlowModel.enhance_long`; for a
ScoreModel or a RegressionModel the same machinery, `_WaveModel._enhance_long`) on the concatenated input.

Decoded audio arrives a block at a time and enhanced audio leaves with a bounded delay; several such streams share one model.  A
session runs the rows `longform.plan_rows` would cut the finished recording into, each as soon as it can run
(`longform.StreamPlanner`): a row's output depends on (samples, seed, absolute frame) only, every row but the last sits at a fixed
stride, so neither the cut of the input into pushes nor the other sessions in a native call leave a trace in the output.

One `StreamPool.step()` is one table upload and three native calls whatever the number of sessions (include/flowdec_hip.h "Streaming"):
fd_stream_gather (the sessions' rings -> the rows of the call, the causal factors), the model class's chunks call (fd_enhance_chunks,
fd_score_enhance_chunks or fd_regression_enhance_chunks: `model._chunks_call`), fd_stream_emit (finished samples out, cross-faded against
the tail each session carries; the next tail stored).  The regression model makes ONE network evaluation per row: the lowest-latency
post-filter a stream can have.

Geometry, with h = hop, rf = row_frames, halo = halo_frames, half = xfade / 2:  W = rf * h - 1, S = (rf - 2 * halo - 1) * h.  Worst-case
algorithmic delay: a sample leaves once (rf - halo) * h + half further samples have arrived (`StreamPool.delay_samples`), plus one
row's compute time.  Device memory per session: a ring of S + W input samples and two tails of xfade samples.

Normalisation cannot be the recording's maximum (it is not known yet): `normfac` is a fixed float, or "causal" -- a row is scaled by the
peak of everything up to its end, `enhance_long(..., normfac="causal")`.  A normalize_mode='none' model takes normfac=None.
"""
import contextlib
import ctypes as C
from typing import Dict, Optional

import numpy as np
import torch

from . import _lib as L
from . import longform
from . import noise as fd_noise
from . import ops
from . import resample as R
from .model import _serialized


def _check_args(model, normfac, capacity):
    """The refusals that need no GPU (the sampler's are the model's: `_chunks_call`).  -> normfac as None, 'causal' or a positive float."""
    if int(capacity) < 1:
        raise ValueError(f"StreamPool: capacity must be >= 1 (got {capacity})")
    if model.normalize_mode == "noisy":
        if normfac is None:
            raise ValueError("StreamPool: a normalize_mode='noisy' model needs normfac=<float> or normfac='causal' -- the recording's "
                             "maximum is not known while it streams")
        if isinstance(normfac, str):
            if normfac != "causal":
                raise ValueError(f"StreamPool: normfac is a float or 'causal' (got {normfac!r})")
            return normfac
        normfac = float(normfac)
        if not (np.isfinite(normfac) and normfac > 0):
            raise ValueError(f"StreamPool: normfac must be positive and finite (got {normfac})")
        return normfac
    if normfac is not None:
        raise ValueError("StreamPool: normfac needs normalize_mode='noisy' (a 'none' model does not normalise)")
    return None


class _Session:
    def __init__(self, sid, slot, seed, planner):
        self.sid, self.slot, self.seed, self.planner = sid, slot, seed, planner
        self.queue = []            # pushed blocks (float32, 1-D) that did not fit the ring yet
        self.fed = 0               # samples written to the ring so far (absolute)


class StreamPool:
    """Up to `capacity` concurrent streaming sessions on one model: a FlowModel, a ScoreModel or a RegressionModel.

        pool = StreamPool(model, capacity=8, N=6, solver="euler", row_frames=256, halo_frames=64, normfac="causal")
        sid = pool.open(seed=7)
        pool.push(sid, block)                 # float32 or int16 (x * 2^-15), CPU or device, any size
        for sid, x in pool.step().items(): ...   # ONE native call over every session that has a row ready (at most one row each)
        tail = pool.flush(sid)                # the rest of the stream; closes the session

    Concatenated, what `step` and `flush` return for a session equals `model.enhance_long(all its input, seed=seed, normfac=normfac,
    same geometry)` bit for bit.  Outputs are float32 tensors on the model's device.  `native_calls` counts the chunks calls,
    `rows_run` the rows they carried.  The buffers of every batch size B live as long as the pool, so each B captures its hipGraph once.

    All sessions of a pool share ONE sampler configuration.  A flow model takes `N`, `solver`, `sigma_fac` (None: N = 50, 'euler', 1.0);
    a score model takes `N` (None: 30) and, in place of `solver`, the arguments of its predictor-corrector sampler as keywords --
    predictor, corrector, corrector_steps, snr, denoise --, and refuses `solver` / `sigma_fac`; a regression model takes none of them, and
    `open` ignores its seed."""

    def __init__(self, model, capacity: int = 8, N: Optional[int] = None, solver: Optional[str] = None, sigma_fac: Optional[float] = None,
                 row_frames: int = 3712, halo_frames: int = 256, xfade: Optional[int] = None, normfac="causal", use_graph: bool = True, **sampler):
        sampler.update({k: v for k, v in dict(N=N, solver=solver, sigma_fac=sigma_fac).items() if v is not None})
        self._call = model._chunks_call(who="StreamPool", **sampler)      # the sampler's refusals; what a step issues between gather and emit
        self.normfac = _check_args(model, normfac, capacity)
        self.model, self.backbone = model, model.backbone      # (.backbone: what @_serialized locks)
        self.capacity, self.sampler, self.use_graph = int(capacity), sampler, bool(use_graph)
        self.dev = model.device
        if self.dev.type != "cuda":
            raise RuntimeError("flowdec_amd: move the model to the GPU first (`model.cuda()`)")
        lib = L.load()
        self.cfg = model.feature_extractor._cfg()
        hop = self.cfg["hop"]
        self.geom = longform.StreamPlanner(hop, row_frames, halo_frames, xfade)       # argument checks; never pushed to
        self.rf, self.halo, self.xfade, self.W = self.geom.rf, self.geom.halo, self.geom.xfade, self.geom.W
        self.Tp = int(lib.fd_padded_frames(self.rf))
        assert hop * self.Tp - 1 == self.W
        self.delay_samples = self.geom.delay_samples
        self.ring_cap = self.geom.ring_samples
        self.native_calls = self.rows_run = 0
        self._sessions: Dict[int, _Session] = {}
        self._free = list(range(self.capacity))[::-1]
        self._next_sid = 0
        self._io = {}
        with torch.cuda.device(self.dev):
            self._rings = torch.zeros(self.capacity, self.ring_cap, dtype=torch.float32, device=self.dev)
            self._tails = torch.zeros(self.capacity, 2, max(self.xfade, 1), dtype=torch.float32, device=self.dev)
            self._peak = torch.zeros(self.capacity, dtype=torch.float32, device=self.dev)
            self._weights = torch.from_numpy(longform.stitch_weights(self.xfade)).to(self.dev) if self.xfade else None

    # -- sessions ------------------------------------------------------------------------------------------------------------
    @_serialized
    def open(self, seed=None) -> int:
        """A new session.  `seed` as `enhance_long(seed=)` of a one-channel recording: an int s means clip_seed(s, 0); [s] or an int64 /
        uint64 tensor [1] gives the 64-bit seed directly.  A regression model draws no noise: its sessions need none."""
        if not self._free:
            raise RuntimeError(f"StreamPool: all {self.capacity} sessions are open")
        seed64 = int(fd_noise.seeds_to_tensor(seed, 1, "cpu")[0]) if self.model._draws_noise else 0
        slot = self._free.pop()
        sid, self._next_sid = self._next_sid, self._next_sid + 1
        self._sessions[sid] = _Session(sid, slot, seed64, longform.StreamPlanner(self.geom.hop, self.rf, self.halo, self.xfade, t_pad=self.Tp))
        with self._side():
            self._peak[slot].zero_()
        return sid

    def _session(self, sid) -> _Session:
        if sid not in self._sessions:
            raise KeyError(f"StreamPool: no open session {sid!r}")
        return self._sessions[sid]

    @torch.no_grad()
    def push(self, sid: int, x) -> None:
        """Append samples to a session: float32, or int16 PCM (converted as x * 2^-15, exact); a tensor or array of any shape (flattened),
        on the CPU or the model's device.  Host bookkeeping only: the block is copied (the caller may reuse its buffer; a device block on
        the caller's current stream) and waits in the session's queue until `step` / `flush` move it into the ring -- one copy per
        session and step however many pushes it took.  Push and step from the same stream (or order them yourself)."""
        s = self._session(sid)
        x = torch.as_tensor(x).reshape(-1)
        if x.is_cuda and x.device != self.dev:
            raise RuntimeError(f"StreamPool.push: the block lives on {x.device}, the model on {self.dev}")
        if x.dtype == torch.int16:
            x = x.to(torch.float32) * (1.0 / 32768.0)
        elif x.dtype == torch.float32:
            x = x.clone()
        else:
            raise TypeError(f"StreamPool.push: float32 or int16 samples (got {x.dtype})")
        if x.numel() == 0:
            return
        s.planner.push(x.numel())                       # refuses past 2^31 absolute frames
        s.queue.append(x)

    def _feed(self, s: _Session) -> None:
        """Queue -> ring, as far as the retention invariant allows: the ring holds [retain_from, fed), at most ring_cap samples.  What is
        taken goes over as ONE block -- a plain copy (two on wrap), on the side stream: ordered after the gather that last read what it
        overwrites."""
        cap = self.ring_cap
        room = s.planner.retain_from + cap - s.fed
        pieces = []
        while s.queue and room > 0:
            x = s.queue[0]
            if x.numel() <= room:
                pieces.append(s.queue.pop(0))
            else:
                pieces.append(x[:room])
                s.queue[0] = x[room:]
            room -= pieces[-1].numel()
        if not pieces:
            return
        if len(pieces) > 1:
            if any(p.is_cuda for p in pieces):
                pieces = [p.to(self.dev) for p in pieces]
            pieces = [torch.cat(pieces)]
        x, ring = pieces[0], self._rings[s.slot]
        if not x.is_cuda:
            x = x.pin_memory()                          # (caching host allocator: the block outlives the asynchronous copy)
        pos = s.fed % cap
        k0 = min(x.numel(), cap - pos)
        ring[pos:pos + k0].copy_(x[:k0], non_blocking=True)
        if x.numel() > k0:
            ring[:x.numel() - k0].copy_(x[k0:], non_blocking=True)
        s.fed += x.numel()

    @torch.no_grad()
    @_serialized
    def _step(self) -> Dict[int, torch.Tensor]:
        with self._side() as h:
            ready = []
            for s in self._sessions.values():
                if s.planner.ready():
                    self._feed(s)
                    ready.append((s, s.planner.next_row()))
            outs = self._run(ready, self.W, h)
        return self._hand_over(outs)

    def step(self) -> Dict[int, torch.Tensor]:
        """ONE native call over every session that has a regular row ready, at most one row per session -> {sid: the samples that row
        finished}; {} when no session is ready (host bookkeeping only: nothing is enqueued, no lock taken)."""
        if not any(s.planner.ready() for s in self._sessions.values()):
            return {}
        return self._step()

    def flush(self, sid: int) -> torch.Tensor:
        """End a session: runs the rows it still has ready (one native call each) and its last row -> everything not returned yet.  The
        session is closed and its slot freed."""
        return self.flush_many([sid])[sid]

    @torch.no_grad()
    @_serialized
    def flush_many(self, sids) -> Dict[int, torch.Tensor]:
        """`flush` for several sessions that end together: their rows share native calls (still at most one row per session per call)."""
        lib, hop = L.load(), self.geom.hop
        ss = [self._session(sid) for sid in dict.fromkeys(sids)]
        outs = {s.sid: [] for s in ss}
        try:
            with self._side() as h:
                while True:                                      # the regular rows that are still ready
                    ready = []
                    for s in ss:
                        if s.planner.ready():
                            self._feed(s)
                            ready.append((s, s.planner.next_row()))
                    if not ready:
                        break
                    for sid, o in self._run(ready, self.W, h).items():
                        outs[sid].append(o)
                last = {}                                        # the last rows, by bucket: a recording of ONE row runs in the bucket of its
                for s in ss:                                     # own length, as enhance_long runs it
                    if s.planner.n == 0:
                        continue
                    self._feed(s)
                    r = s.planner.flush()
                    assert not s.queue and s.fed == s.planner.n
                    Tp = int(lib.fd_padded_frames(lib.fd_num_frames(r.row.length, hop))) if r.index == 0 else self.Tp
                    ops.check_ragged_lengths([r.row.length], hop * Tp - 1, self.cfg["n_fft"], hop)
                    last.setdefault(hop * Tp - 1, []).append((s, r))
                for Lrow, ready in last.items():
                    for sid, o in self._run(ready, Lrow, h).items():
                        outs[sid].append(o)
                res = {sid: torch.cat(o) if o else torch.empty(0, dtype=torch.float32, device=self.dev) for sid, o in outs.items()}
        finally:
            for s in ss:
                self._close(s)
        return self._hand_over(res)

    def _close(self, s: _Session) -> None:
        del self._sessions[s.sid]
        self._free.append(s.slot)

    # -- the native step ----------------------------------------------------------------------------------------------------------
    @contextlib.contextmanager
    def _side(self):
        """The model's side stream, ordered after / before the caller's current stream.  -> the model's native handle."""
        h = self.model._sync_native()
        with torch.cuda.device(self.dev), self.model._on_side_stream(self.dev):
            yield h

    def _hand_over(self, outs):
        cur = torch.cuda.current_stream(self.dev)
        for o in outs.values():
            o.record_stream(cur)
        return outs

    def _buffers(self, B, Lrow):
        """The device arrays of the native calls at batch size B.  They live as long as the pool: a captured graph is keyed on them."""
        key = (B, Lrow)
        if key not in self._io:
            dev = self.dev
            io = dict(y=torch.zeros(B, Lrow, dtype=torch.float32, device=dev), out=torch.empty(B, Lrow, dtype=torch.float32, device=dev),
                      fin=torch.empty(B, Lrow, dtype=torch.float32, device=dev), normfac=torch.ones(B, dtype=torch.float32, device=dev),
                      table=torch.zeros(B * (C.sizeof(L.FdStreamRow) + 16), dtype=torch.uint8, device=dev))    # rows | seeds | lens | frame0
            if isinstance(self.normfac, float):
                io["normfac"].fill_(self.normfac)
            self._io[key] = io
        return self._io[key]

    def _run(self, ready, Lrow, h):
        """gather -> the model's chunks call -> emit over `ready` = [(session, StreamRow)] -> {sid: finished samples}.  Inside `_side()`, whose
        model handle is `h`."""
        lib, dev, B, X, half = L.load(), self.dev, len(ready), self.xfade, self.xfade // 2
        io = self._buffers(B, Lrow)
        rows = (L.FdStreamRow * B)()
        for b, (s, sr) in enumerate(ready):
            r, (f0, f1) = sr.row, sr.finished
            e = rows[b]
            e.ring, e.start, e.ring_cap, e.length, e.peak_slot = self._rings[s.slot].data_ptr(), r.start, self.ring_cap, r.length, s.slot
            e.emit_lo, e.emit_count = f0 - r.start, f1 - f0
            e.tail_lo = 0 if sr.last else r.xfade_hi - half - r.start
            e.tail_in = self._tails[s.slot, (sr.index - 1) % 2].data_ptr() if X and sr.index > 0 else None
            e.tail_out = self._tails[s.slot, sr.index % 2].data_ptr() if X and not sr.last else None
            e.out = io["fin"][b].data_ptr()
            # what the kernels trust: the row lies in the ring, the finished range and the tail inside the row
            assert s.planner.retain_from <= r.start and r.start + r.length <= s.fed <= r.start + self.ring_cap and 1 <= r.length <= Lrow
            assert 0 <= e.emit_lo and e.emit_lo + e.emit_count <= r.length and (sr.last or 0 <= e.tail_lo and e.tail_lo + X <= r.length)
        nrow = B * C.sizeof(L.FdStreamRow)
        host = np.concatenate([np.frombuffer(bytes(rows), dtype=np.uint8),
                               np.array([s.seed for s, _ in ready], dtype=np.int64).view(np.uint8),
                               np.array([sr.row.length for _, sr in ready], dtype=np.int32).view(np.uint8),
                               np.array([sr.row.frame0 for _, sr in ready], dtype=np.int32).view(np.uint8)])
        # the step's ONE upload, from pinned memory of torch's caching host allocator (which keeps the block until the copy has run): the host
        # does not wait for the device here, so the next step is enqueued while this one computes
        io["table"].copy_(torch.from_numpy(host).pin_memory(), non_blocking=True)
        tp = io["table"].data_ptr()
        table, seeds, lens, frame0 = (C.c_void_p(tp + o) for o in (0, nrow, nrow + 8 * B, nrow + 12 * B))
        causal = self.normfac == "causal"
        L.check(lib.fd_stream_gather(table, B, L.ptr(io["y"]), Lrow, L.ptr(self._peak) if causal else None,
                                     L.ptr(io["normfac"]) if causal else None, L.stream()))
        need = lib.fd_enhance_workspace_bytes(h, B, Lrow)
        need_cap = lib.fd_enhance_workspace_bytes(h, self.capacity, self.W)      # ONE workspace for every B: its address keys the graphs
        if need == 0 or need_cap == 0:
            raise RuntimeError("flowdec_hip: " + lib.fd_last_error().decode())
        ws = self.backbone.workspace(("enh", self.capacity, self.W), max(need, need_cap), dev)
        self._call(lib, h, L.ptr(io["y"]), lens, seeds, frame0, L.ptr(io["normfac"]) if self.normfac is not None else None, L.ptr(io["out"]), B, Lrow,
                   ws, self.use_graph)
        L.check(lib.fd_stream_emit(table, B, L.ptr(io["out"]), Lrow, L.ptr(self._weights), X, L.stream()))
        self.native_calls += 1
        self.rows_run += B
        return {s.sid: io["fin"][b, :sr.finished[1] - sr.finished[0]].clone() for b, (s, sr) in enumerate(ready)}


class EnhanceStream:
    """One stream: a `StreamPool` of one session.

        st = EnhanceStream(model, seed=7, N=6, solver="euler", row_frames=256, halo_frames=64, normfac="causal")
        for block in blocks: out.append(st.push(block))     # whatever became final (often empty)
        out.append(st.flush())                               # torch.cat(out) == model.enhance_long(cat(blocks), seed=7, normfac="causal", ...)

    `model` is any of the three classes; `pool_kwargs` carry its sampler as `StreamPool` takes it (a regression model needs no seed).

    `in_rate` / `out_rate` (Hz; None or the model's rate: as above) put a `resample.ResampleStream` in front of the pool and one behind
    it: the concatenated output is then R_out(model.enhance_long(R_in(all input), ...)) bit for bit, R = `resample.resample_device` at
    lowpass_filter_width 64, however the input was cut.  `delays` = (resampler in, pool, resampler out) in samples at the input rate,
    the model's rate and the model's rate; `delay_samples` stays the pool's."""

    def __init__(self, model, seed=None, in_rate: Optional[int] = None, out_rate: Optional[int] = None, **pool_kwargs):
        self.pool = StreamPool(model, capacity=1, **pool_kwargs)
        self.sid = self.pool.open(seed)
        self.delay_samples = self.pool.delay_samples
        sr = int(model.sampling_rate)
        self.in_rate, self.out_rate = int(in_rate or sr), int(out_rate or sr)
        self._rin = R.ResampleStream(R.get_resampler(self.in_rate, sr, device=self.pool.dev)) if self.in_rate != sr else None
        self._rout = R.ResampleStream(R.get_resampler(sr, self.out_rate, device=self.pool.dev)) if self.out_rate != sr else None
        self.delays = (self._rin.delay_samples if self._rin else 0, self.delay_samples, self._rout.delay_samples if self._rout else 0)

    def push(self, x) -> torch.Tensor:
        if self._rin is not None:
            x = self._rin.push(x)
        self.pool.push(self.sid, x)
        outs = []
        while True:
            got = self.pool.step()
            if not got:
                break
            outs.append(got[self.sid])
        y = torch.cat(outs) if outs else torch.empty(0, dtype=torch.float32, device=self.pool.dev)
        return self._rout.push(y) if self._rout is not None else y

    def flush(self) -> torch.Tensor:
        if self._rin is not None:
            self.pool.push(self.sid, self._rin.flush())
        y = self.pool.flush(self.sid)
        if self._rout is not None:
            y = torch.cat([self._rout.push(y), self._rout.flush()])
        return y
