"""Codec session pools: many NDAC streaming sessions through ONE native call per step (include/flowdec_hip.h "Codec pools").

`ndac_stream.DecodeStream` / `EncodeStream` serve one session per call, and a push costs the ~32 launches of a window whatever the block.
A pool keeps every session's input in a device ring, lets `ndac_stream.DecodePlanner` (one per session, unchanged) decide which windows
are ready, and runs the ready windows of ALL sessions as the rows of one fd_ndac_pool_decode / fd_ndac_pool_encode: one table upload,
one call, a launch count that does not depend on the number of rows, no synchronisation -- and, with `use_graph`, one graph replay.

The promise is the streams': concatenated, what a session gets back is `dac.decode(dac.quantizer.from_codes(all its codes)[0])[0, 0]`
resp. `dac.encode(dac.preprocess(all its samples), nq)[1][0]` bit for bit, however the input was cut into pushes, whichever sessions
shared its calls, with or without the graph, in every precision mode (a ragged row is its one-clip result; DESIGN.md section 2 "Codec pools").

Geometry, with (hl, hr) the codec's halo and b = block_frames: every call has T = hl + b + hr frames per row -- shorter first and last
windows are rows with fewer frames -- so a step's shape is (rows, precision) only; a session's ring holds hl + 2 b + hr - 1 frames (what
the planner can still ask for plus one block); input that does not fit yet waits in a host-side queue.
"""
import contextlib
import ctypes as C
from typing import Dict, List, Optional

import numpy as np
import torch

from . import _lib as L
from .ndac_stream import DecodePlanner, Job, _as_code_rows, _samples_per_frame
from .stream import StreamPool


def _require_gpu(dac) -> torch.device:
    if dac.device.type != "cuda":
        raise RuntimeError("flowdec_amd.ndac: the codec must be on the GPU (`dac_model.to('cuda')`); there is no CPU path")
    return dac.device


def _native(pool, rows, B: int, T: int, nq_call: int) -> None:
    """The step's ONE upload and ONE native call over `rows` (a ctypes array of B FdNdacPoolRow, also the host copy the call checks).
    Runs on the pool's side stream.  Raises -- with nothing launched -- when the call refuses the table."""
    lib, dac = L.load(), pool.dac
    with dac._lock:
        h = dac.handle()
        dac._apply_precision(h)
        if pool._ws is None:
            need = lib.fd_ndac_pool_workspace_bytes(h, pool.capacity, T)
            if need == 0:
                raise RuntimeError("flowdec_hip: " + (lib.fd_last_error() or b"fd_ndac_pool_workspace_bytes refused the shape").decode())
            pool._ws = torch.empty(need, dtype=torch.uint8, device=pool.dev)      # ONE workspace for every B: its address keys the graphs
        # from pinned memory of torch's caching host allocator (which keeps the block until the copy has run): the host does not wait
        nbytes = B * C.sizeof(L.FdNdacPoolRow)
        pool._table[:nbytes].copy_(torch.from_numpy(np.frombuffer(bytes(rows), dtype=np.uint8).copy()).pin_memory(), non_blocking=True)
        args = (h, L.ptr(pool._table), rows, B, T)
        tail = (L.ptr(pool._ws), pool._ws.numel(), int(pool.use_graph), L.stream())
        L.check(lib.fd_ndac_pool_encode(*args, nq_call, *tail) if pool.ENCODE else lib.fd_ndac_pool_decode(*args, *tail))


class _Session:
    def __init__(self, sid: int, slot: int, nq: int, planner: DecodePlanner):
        self.sid, self.slot, self.nq, self.planner = sid, slot, nq, planner
        self.queue: List[torch.Tensor] = []   # pushed pieces [rows, n] that are not in the ring yet
        self.fed = 0                          # ring units (decode: frames, encode: samples) written so far, absolute
        self.received = 0                     # ring units pushed so far
        self.hold: Optional[int] = None       # first frame a planned job that has not run yet still reads: the ring keeps it
        self.ending = self.padded = False


class _CodecPool:
    """What DecodePool and EncodePool share: sessions, rings, the step.  `unit`: ring elements per frame."""
    ENCODE = False

    def __init__(self, dac, capacity: int, block_frames: int, use_graph: bool, halo, unit: int, ring_rows: int, ring_dtype, out_per_frame: int, out_dtype):
        who = type(self).__name__
        if int(capacity) < 1:
            raise ValueError(f"{who}: capacity must be >= 1 (got {capacity})")
        self.dac, self.capacity, self.use_graph, self.unit = dac, int(capacity), bool(use_graph), int(unit)
        self.geom = DecodePlanner(halo[0], halo[1], block_frames)           # argument checks; never pushed to
        self.halo_left, self.halo_right, self.block = self.geom.halo_left, self.geom.halo_right, self.geom.block
        self.T = self.halo_left + self.block + self.halo_right              # frames per row of EVERY call
        self.ring_frames = self.geom.max_buffered + self.block
        self.ring_cap = self.ring_frames * self.unit
        self.emit_max = self.block + self.halo_right                         # a row finishes a block, or a flush's rest (fewer than this)
        self.native_calls = self.rows_run = 0
        self._sessions: Dict[int, _Session] = {}
        self._free = list(range(self.capacity))[::-1]
        self._next_sid = 0
        self._ws = self._stream = None
        dev = self.dev
        self._rings = torch.zeros(self.capacity, ring_rows, self.ring_cap, dtype=ring_dtype, device=dev)
        self._fin = torch.zeros(self.capacity, out_per_frame * self.emit_max, dtype=out_dtype, device=dev)
        self._table = torch.zeros(self.capacity * C.sizeof(L.FdNdacPoolRow), dtype=torch.uint8, device=dev)

    # -- sessions ------------------------------------------------------------------------------------------------------------
    def _open(self, nq: int) -> int:
        who = type(self).__name__
        if not 1 <= int(nq) <= self.dac.n_codebooks:
            raise RuntimeError(f"{who}: {nq} code rows but the model has {self.dac.n_codebooks} codebooks")
        if not self._free:
            raise RuntimeError(f"{who}: all {self.capacity} sessions are open")
        sid, self._next_sid = self._next_sid, self._next_sid + 1
        # (a reused slot keeps the old ring's content: a window never reaches outside [keep_from, fed) of its OWN session)
        self._sessions[sid] = _Session(sid, self._free.pop(), int(nq), DecodePlanner(self.halo_left, self.halo_right, self.block))
        return sid

    def _session(self, sid) -> _Session:
        if sid not in self._sessions:
            if isinstance(sid, int) and 0 <= sid < self._next_sid:
                raise RuntimeError(f"{type(self).__name__}: session {sid} has been flushed (push or flush after flush)")
            raise KeyError(f"{type(self).__name__}: no open session {sid!r}")
        return self._sessions[sid]

    def _enqueue(self, s: _Session, x: torch.Tensor) -> None:
        if s.ending:
            raise RuntimeError(f"{type(self).__name__}: push after flush")
        if x.is_cuda and x.device != self.dev:
            raise RuntimeError(f"{type(self).__name__}.push: the block lives on {x.device}, the codec on {self.dev}")
        if x.shape[1]:
            s.queue.append(x.clone())          # (the caller may reuse its buffer)
            s.received += x.shape[1]

    def end(self, sid: int) -> None:
        """No more input for this session: the next `step` runs what it still has ready together with the other sessions' rows, its
        last (short) window included, and frees the slot once that has run.  `flush` = `end` + the steps of this session alone."""
        self._session(sid).ending = True

    # -- queue -> ring, ring -> jobs -----------------------------------------------------------------------------------------------
    def _feed(self, s: _Session) -> List[Job]:
        """Moves as much of the queue into the ring as it can hold -- it keeps [keep, fed), keep = the first frame a job can still read -- as
        ONE block (two copies on wrap) and tells the planner about the whole frames that arrived.  -> the jobs that became ready."""
        keep = s.planner.keep_from if s.hold is None else min(s.hold, s.planner.keep_from)
        room = keep * self.unit + self.ring_cap - s.fed
        pieces = []
        while s.queue and room > 0:
            x = s.queue[0]
            if x.shape[1] <= room:
                pieces.append(s.queue.pop(0))
            else:
                pieces.append(x[:, :room])
                s.queue[0] = x[:, room:]
            room -= pieces[-1].shape[1]
        if pieces:
            if len(pieces) > 1 and any(p.is_cuda for p in pieces):
                pieces = [p.to(self.dev) for p in pieces]
            x = pieces[0] if len(pieces) == 1 else torch.cat(pieces, dim=1)
            if not x.is_cuda and self.dev.type == "cuda":
                x = x.contiguous().pin_memory()
            ring, cap = self._rings[s.slot, :x.shape[0]], self.ring_cap
            pos, n = s.fed % cap, x.shape[1]
            k0 = min(n, cap - pos)
            ring[:, pos:pos + k0].copy_(x[:, :k0], non_blocking=True)
            if n > k0:
                ring[:, :n - k0].copy_(x[:, k0:], non_blocking=True)
            s.fed += n
        jobs = s.planner.push(s.fed // self.unit - s.planner.received)
        if jobs and s.hold is None:
            s.hold = jobs[0][0]
        return jobs

    def _last_input(self, s: _Session) -> None:
        """What an ending session adds to its queue before its last window (encode: the zero padding of a trailing partial frame)."""

    def _collect(self, sessions) -> list:
        """-> [(session, job)] of everything that can run now, in session order, per session in stream order."""
        ready = []
        for s in sessions:
            jobs = self._feed(s)
            if s.ending and not s.queue and not s.planner.closed:
                if not s.padded:
                    s.padded = True
                    self._last_input(s)
                    jobs += self._feed(s)
                if not s.queue:
                    jobs += s.planner.flush()
            ready += [(s, j) for j in jobs]
        return ready

    # -- the native step ----------------------------------------------------------------------------------------------------------
    @contextlib.contextmanager
    def _on_side(self):
        """Stream capture is illegal on the legacy default stream: everything the pool puts on the device runs on its own stream, ordered
        after / before the caller's current stream (yielded, for the `record_stream` of what the caller gets back)."""
        if self.dev.type != "cuda":
            yield None
            return
        with torch.cuda.device(self.dev):
            cur = torch.cuda.current_stream(self.dev)
            if self._stream is None:
                self._stream = torch.cuda.Stream(self.dev)
            self._stream.wait_stream(cur)
            with torch.cuda.stream(self._stream):
                yield cur
            cur.wait_stream(self._stream)

    def _rows(self, ready):
        """The table of one call.  -> (ctypes rows, n_quantizers of the call)."""
        rows = (L.FdNdacPoolRow * len(ready))()
        stride = self._fin.shape[1] * self._fin.element_size()
        for b, (s, (w0, w1, e0, e1)) in enumerate(ready):
            r = rows[b]
            r.ring, r.start, r.ring_cap, r.frames, r.nq = self._rings[s.slot].data_ptr(), w0 * self.unit, self.ring_cap, w1 - w0, s.nq
            r.emit_lo, r.emit_count, r.out = e0 - w0, e1 - e0, self._fin.data_ptr() + b * stride
            # what the kernels trust: the window lies in the ring and holds real input, the final frames lie in the window and fit `out`
            assert s.fed - self.ring_cap <= w0 * self.unit and w1 * self.unit <= s.fed and 1 <= w1 - w0 <= self.T
            assert w0 <= e0 <= e1 <= w1 and e1 - e0 <= self.emit_max
        return rows, max(s.nq for s, _ in ready)

    def _call(self, rows, B: int, nq_call: int) -> torch.Tensor:
        """One native call -> a copy of the rows' outputs [B, ...] (one launch whatever B)."""
        _native(self, rows, B, self.T, nq_call)      # T: ALWAYS the full window length, so a step's shape is (B, precision) only
        self.native_calls += 1
        self.rows_run += B
        return self._fin[:B].long() if self.ENCODE else self._fin[:B].clone()

    def _run(self, sessions) -> Dict[int, torch.Tensor]:
        with torch.no_grad(), self._on_side() as cur:
            ready = self._collect(sessions)
            parts: Dict[int, list] = {}
            for g in range(0, len(ready), self.capacity):
                grp = ready[g:g + self.capacity]
                rows, nq_call = self._rows(grp)
                fin = self._call(rows, len(grp), nq_call)
                for b, (s, (_, _, e0, e1)) in enumerate(grp):
                    parts.setdefault(s.sid, []).append(self._cut(fin[b], s, e1 - e0))
            outs = {}
            for s in sessions:
                s.hold = None
                if s.sid in parts:
                    p = parts[s.sid]
                    outs[s.sid] = p[0] if len(p) == 1 else torch.cat(p, dim=-1)
                if s.planner.closed:
                    del self._sessions[s.sid]
                    self._free.append(s.slot)
        if cur is not None:
            for o in outs.values():
                o.record_stream(cur)
        return outs

    def step(self) -> Dict[int, torch.Tensor]:
        """ONE native call over every window that is ready, of every session, in session order (more than `capacity` rows: further calls)
        -> {sid: what became final}; {} when nothing was ready (then every pushed block is in its ring)."""
        return self._run(list(self._sessions.values()))

    def flush(self, sid: int) -> torch.Tensor:
        """End a session -> everything not returned yet; frees the slot."""
        s = self._session(sid)
        self.end(sid)
        parts = []
        while sid in self._sessions:
            got = self._run([s])
            if sid in got:
                parts.append(got[sid])
        return torch.cat(parts, dim=-1) if parts else self._empty(s)


class DecodePool(_CodecPool):
    """Up to `capacity` concurrent streaming decode sessions on one `DAC` (on the GPU, even decoder rates).

        pool = DecodePool(dac, capacity=32, block_frames=1, use_graph=True)
        sid = pool.open(n_quantizers=10)           # per session; sessions of one pool may differ
        pool.push(sid, codes)                      # [nq, n] integers, any n >= 0, host or device
        outs = pool.step()                         # {sid: float32 1-D}: ONE native call over every window that is ready
        tail = pool.flush(sid)                     # the rest of the stream; frees the slot

    Concatenated, a session's outputs are `dac.decode(dac.quantizer.from_codes(all its codes)[0])[0, 0]` bit for bit.  `native_calls`
    counts fd_ndac_pool_decode calls, `rows_run` the windows they carried; `delay_samples` as `DecodeStream.delay_samples`."""

    def __init__(self, dac, capacity: int = 32, block_frames: int = 1, use_graph: bool = True):
        self.dev = _require_gpu(dac)
        for r in dac.decoder_rates:
            if int(r) % 2:      # fd_ndac_decode_halo's refusal, before the codec is touched
                raise RuntimeError(f"DecodePool: decoder rate {int(r)} is odd (the decoded length is not frames * hop: no window arithmetic)")
        self.up = _samples_per_frame(dac)
        super().__init__(dac, capacity, block_frames, use_graph, dac.decode_halo(), 1, dac.n_codebooks, torch.int32, self.up, torch.float32)
        self.delay_samples = self.geom.latency_frames * self.up

    def open(self, n_quantizers: int) -> int:
        return self._open(n_quantizers)

    def push(self, sid: int, codes) -> None:
        """Append frames to a session.  Host bookkeeping only: the block is copied and waits in the session's queue until a step moves it
        into the ring.  Push and step from the same stream (or order them yourself)."""
        s = self._session(sid)
        c = _as_code_rows(codes, "DecodePool.push")
        if c.shape[0] != s.nq:
            raise RuntimeError(f"DecodePool.push: {c.shape[0]} code rows, the session has {s.nq}")
        self._enqueue(s, c.to(torch.int32))

    def _cut(self, row, s, count):
        return row[:count * self.up]

    def _empty(self, s):
        return torch.empty(0, dtype=torch.float32, device=self.dev)


class EncodePool(_CodecPool):
    """Up to `capacity` concurrent streaming encode sessions on one `DAC` (on the GPU): `DecodePool`'s shape, samples in, codes out.

        sid = pool.open(n_quantizers=4); pool.push(sid, samples)     # 1-D float32, any length, host or device
        pool.step() / pool.flush(sid)                                # [nq, k] int64 codes

    Concatenated along the frames, a session's outputs are `dac.encode(dac.preprocess(all its samples), nq)[1][0]` bit for bit; `flush`
    zero-pads a trailing partial frame as `DAC.preprocess` does.  A call quantises with the largest nq among its rows; the codes of
    quantiser i do not depend on the later ones, so a session that asked for fewer rows gets exactly its own encode."""
    ENCODE = True

    def __init__(self, dac, capacity: int = 32, block_frames: int = 1, use_graph: bool = True):
        self.dev = _require_gpu(dac)
        self.hop = int(dac.hop_length)
        super().__init__(dac, capacity, block_frames, use_graph, dac.encode_halo(), self.hop, 1, torch.float32, dac.n_codebooks, torch.int32)
        self.delay_samples = self.geom.latency_frames * self.hop

    def open(self, n_quantizers: Optional[int] = None) -> int:
        return self._open(self.dac.n_codebooks if n_quantizers is None else n_quantizers)

    def push(self, sid: int, samples) -> None:
        s = self._session(sid)
        x = torch.as_tensor(samples)
        if x.ndim != 1 or x.dtype != torch.float32:
            raise TypeError(f"EncodePool.push: samples must be 1-D float32 (got {x.dtype}, shape {tuple(x.shape)})")
        self._enqueue(s, x[None])

    def _last_input(self, s):
        part = s.received % self.hop
        if part:                                      # the trailing partial frame, zero-padded as DAC.preprocess pads it
            s.queue.append(torch.zeros(1, self.hop - part, dtype=torch.float32))
            s.received += self.hop - part

    def _cut(self, row, s, count):
        return row[:s.nq * count].view(s.nq, count)

    def _empty(self, s):
        return torch.empty(s.nq, 0, dtype=torch.int64, device=self.dev)


class CodesEnhancePool:
    """`DecodePool` in front of `stream.StreamPool`: code indices in, enhanced audio out, the decoded PCM handed over on the device.

        pool = CodesEnhancePool(model, dac, capacity=8, decode_block_frames=8, N=6, solver="euler", normfac="causal", ...)
        sid = pool.open(seed=7, n_quantizers=10); pool.push(sid, codes); outs = pool.step(); tail = pool.flush(sid)

    Per session the output is what `stream_cli --codes` produces for that stream with the same options, byte for byte."""

    def __init__(self, model, dac, capacity: int = 8, decode_block_frames: int = 8, **stream_pool_kwargs):
        self.codec = DecodePool(dac, capacity=capacity, block_frames=decode_block_frames, use_graph=stream_pool_kwargs.get("use_graph", True))
        self.enhancer = StreamPool(model, capacity=capacity, **stream_pool_kwargs)
        self._enh: Dict[int, int] = {}      # session id (the codec pool's) -> the enhance pool's

    def open(self, seed, n_quantizers: int) -> int:
        e = self.enhancer.open(seed)
        try:
            sid = self.codec.open(n_quantizers)
        except Exception:
            self.enhancer.flush(e)
            raise
        self._enh[sid] = e
        return sid

    def push(self, sid: int, codes) -> None:
        self.codec.push(sid, codes)

    def step(self) -> Dict[int, torch.Tensor]:
        """One decode step, its PCM into the enhance pool, one enhance step -> {sid: enhanced samples}."""
        for sid, pcm in self.codec.step().items():
            self.enhancer.push(self._enh[sid], pcm)
        back = {e: sid for sid, e in self._enh.items()}
        return {back[e]: x for e, x in self.enhancer.step().items()}

    def flush(self, sid: int) -> torch.Tensor:
        e = self._enh.pop(sid)
        self.enhancer.push(e, self.codec.flush(sid))
        return self.enhancer.flush(e)
