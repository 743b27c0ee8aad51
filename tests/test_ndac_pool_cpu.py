"""Codec session pools, host side (flowdec_amd/ndac_pool.py; include/flowdec_hip.h "Codec pools"): nothing here needs a GPU.

The native step is stubbed by a toy codec that has the property the real one has -- a frame's output depends on the frames within the
halo only, with zeros beyond the ends of what it is given -- and that works from the TABLE alone: it reads the rings through the rows'
pointers, start and frames, and writes through `out`.  So a session's concatenated output equals the toy's one-shot result only if rings,
windows, tables, grouping and emission are all right."""
import ctypes as C
import random

import numpy as np
import pytest
import torch

HL, HR, NCB, HOP = 3, 2, 4, 8        # the toy's halo (frames), codebooks and samples per frame (both directions)
TAPS = np.array([3, -1, 4, 1, -5, 9], dtype=np.int64)      # frame f sees frames f - HL .. f + HR


class ToyCodec:
    """Stands in for `flowdec_amd.ndac.DAC` under the pools: geometry only."""
    n_codebooks, hop_length, decoder_rates, encoder_rates, sample_rate = NCB, HOP, (4, 2), (2, 4), 16000
    device = torch.device("cpu")

    def decode_halo(self):
        return HL, HR

    def encode_halo(self):
        return HL, HR


def fir(v):
    """v [n] int64 per-frame values -> per-frame outputs; zeros beyond both ends."""
    p = np.concatenate([np.zeros(HL, np.int64), v, np.zeros(HR, np.int64)])
    return np.array([int(TAPS @ p[f:f + HL + HR + 1]) for f in range(len(v))], dtype=np.int64)


def toy_decode(codes):
    """[nq, n] -> float32 [n * HOP]"""
    y = fir((codes.astype(np.int64) * (np.arange(codes.shape[0])[:, None] + 1)).sum(0))
    return (y[:, None] + np.arange(HOP)[None] * 0.125).astype(np.float32).reshape(-1)


def toy_encode(x, nq):
    """int-valued float32 samples [n * HOP] -> int64 [nq, n]"""
    y = fir(x.reshape(-1, HOP).astype(np.int64).sum(1))
    return np.stack([(y * (q + 1)) % 997 for q in range(nq)])


@pytest.fixture
def pools(monkeypatch):
    from flowdec_amd import ndac_pool as P
    calls = []

    def fake_native(pool, rows, B, T, nq_call):
        rec = dict(B=B, T=T, nq=nq_call, rows=[])
        ring0, fin0 = pool._rings.data_ptr(), pool._fin.data_ptr()
        ring_stride = pool._rings[0].numel() * pool._rings.element_size()
        fin_stride = pool._fin.shape[1] * pool._fin.element_size()
        assert len(rows) == B and 1 <= B <= pool.capacity and T == HL + pool.block + HR
        for b in range(B):
            r = rows[b]
            rec["rows"].append({f: getattr(r, f) for f, _ in type(r)._fields_})
            slot, ob = (r.ring - ring0) // ring_stride, (r.out - fin0) // fin_stride
            assert r.ring == ring0 + slot * ring_stride and r.out == fin0 + ob * fin_stride == fin0 + b * fin_stride
            assert 1 <= r.frames <= T and r.frames * pool.unit <= r.ring_cap == pool.ring_cap and 1 <= r.nq <= nq_call
            assert 0 <= r.emit_lo and r.emit_lo + r.emit_count <= r.frames
            ring = pool._rings[slot].numpy()
            idx = (r.start + np.arange(r.frames * pool.unit)) % r.ring_cap          # the window is (start, frames) alone: it may wrap
            lo, hi = r.emit_lo, r.emit_lo + r.emit_count
            if pool.ENCODE:
                got = toy_encode(ring[0, idx], r.nq)[:, lo:hi]
                pool._fin[ob, :got.size] = torch.from_numpy(got.reshape(-1).astype(np.int32))
            else:
                got = toy_decode(ring[:r.nq, idx])[lo * HOP:hi * HOP]
                pool._fin[ob, :got.size] = torch.from_numpy(got)
        calls.append(rec)

    monkeypatch.setattr(P, "_native", fake_native)
    monkeypatch.setattr(P, "_require_gpu", lambda dac: torch.device("cpu"))
    return P, calls


def cut(rng, total, sizes):
    out, left = [], total
    while left:
        n = min(rng.choice(sizes), left)
        out.append(n)
        left -= n
    return out + [0]


def test_ring_arithmetic_and_wrapping_windows(pools):
    """Frame i of code row q lives at ring[q][i % cap]; a window that wraps is described by its start and length alone."""
    P, calls = pools
    pool = P.DecodePool(ToyCodec(), capacity=2, block_frames=2)
    assert (pool.T, pool.ring_frames, pool.ring_cap, pool.emit_max, pool.delay_samples) == (7, 8, 8, 4, 3 * HOP)
    codes = torch.from_numpy(np.random.default_rng(0).integers(0, 1000, size=(3, 40)))
    sid = pool.open(3)
    outs, pos = [], 0
    for n in (1, 0, 5, 2, 2, 9, 1, 20):
        pool.push(sid, codes[:, pos:pos + n])
        pos += n
        while True:
            got = pool.step()
            if not got:
                break
            outs.append(got[sid])
        s = pool._sessions[sid]
        assert s.fed == pos and not s.queue                                          # a step that returns {} left nothing waiting
        ring = pool._rings[s.slot]
        for i in range(max(s.planner.keep_from, pos - pool.ring_cap), pos):
            assert torch.equal(ring[:3, i % pool.ring_cap], codes[:, i].int()), i
    outs.append(pool.flush(sid))
    assert np.array_equal(torch.cat(outs).numpy(), toy_decode(codes.numpy()))
    rows = [r for c in calls for r in c["rows"]]
    assert sum(r["start"] % 8 + r["frames"] > 8 for r in rows) >= 3, "no window wrapped the ring"
    assert max(r["start"] for r in rows) > 3 * 8                                     # ... several times round
    assert all(c["T"] == 7 for c in calls)


def test_table_of_sessions_at_different_phases(pools):
    """One call carries a first window (true left edge), a mid-stream window and the last window of a one-frame stream (a 1-frame emit);
    the call before it carried two rows of ONE session."""
    P, calls = pools
    pool = P.DecodePool(ToyCodec(), capacity=3, block_frames=2)
    rng = np.random.default_rng(1)
    a, b, c = pool.open(4), pool.open(2), pool.open(1)
    ca, cb, cc = (torch.from_numpy(rng.integers(0, 1000, size=(nq, n))) for nq, n in ((4, 4), (2, 8), (1, 1)))
    pool.push(b, cb[:, :6])                # frames [0, 2) and [2, 4) are final: two windows
    first = pool.step()
    assert set(first) == {b} and len(calls) == 1 and (calls[0]["B"], pool.native_calls, pool.rows_run) == (2, 1, 2)
    r0, r1 = calls[0]["rows"]
    assert r0["ring"] == r1["ring"] and r0["out"] != r1["out"]
    assert [(r["start"], r["frames"], r["emit_lo"], r["emit_count"]) for r in (r0, r1)] == [(0, 4, 0, 2), (0, 6, 2, 2)]
    pool.push(a, ca)                       # block + right halo frames: the first window
    pool.push(b, cb[:, 6:])
    pool.push(c, cc)
    pool.end(c)
    got = pool.step()
    assert set(got) == {a, b, c} and len(calls) == 2 and (calls[1]["B"], calls[1]["T"], pool.native_calls, pool.rows_run) == (3, 7, 2, 5)
    rows = calls[1]["rows"]
    assert [(r["start"], r["frames"], r["nq"], r["emit_lo"], r["emit_count"]) for r in rows] == [(0, 4, 4, 0, 2), (1, 7, 2, 3, 2), (0, 1, 1, 0, 1)]
    assert len({r["ring"] for r in rows}) == 3 and all(r["ring_cap"] == 8 for r in rows)
    assert c not in pool._sessions and pool._free == [2] and set(pool._sessions) == {a, b}
    assert np.array_equal(got[c].numpy(), toy_decode(cc.numpy()))
    assert np.array_equal(got[a].numpy(), toy_decode(ca.numpy())[:2 * HOP])
    assert np.array_equal(torch.cat([first[b], got[b], pool.flush(b)]).numpy(), toy_decode(cb.numpy()))


@pytest.mark.parametrize("block", [1, 2, 5])
def test_streams_equal_one_shot_whatever_the_cuts_and_the_company(pools, block):
    """Five sessions through three slots, random cuts (empty pushes, pushes of several ring lengths): every session's output is the toy's
    one-shot decode; calls carry at most `capacity` rows; per session the windows run in stream order."""
    P, calls = pools
    rng, nprng = random.Random(block), np.random.default_rng(block)
    pool = P.DecodePool(ToyCodec(), capacity=3, block_frames=block)
    streams = [(nq, torch.from_numpy(nprng.integers(0, 1000, size=(nq, n)))) for nq, n in ((4, 75), (1, 1), (2, 0), (3, 31), (4, block + HR))]
    waiting, live, outs = list(enumerate(streams)), {}, {}
    while waiting or live:
        while waiting and pool._free:
            k, (nq, codes) = waiting.pop(0)
            sid = pool.open(nq)
            live[sid] = (k, codes, cut(rng, codes.shape[1], [0, 1, 2, 3, 7, 11, 40]), 0)
            outs[k] = []
        if not pool._free and waiting:
            with pytest.raises(RuntimeError, match="sessions are open"):
                pool.open(1)
        for sid in list(live):
            k, codes, cuts, pos = live[sid]
            n = cuts.pop(0)
            pool.push(sid, codes[:, pos:pos + n] if rng.random() < 0.5 else codes[None, :, pos:pos + n])
            live[sid] = (k, codes, cuts, pos + n)
        for sid, y in pool.step().items():
            outs[live[sid][0]].append(y)
        assert pool.native_calls == len(calls) and pool.rows_run == sum(c["B"] for c in calls)
        for sid in [s for s in live if not live[s][2]]:
            outs[live.pop(sid)[0]].append(pool.flush(sid))
    for k, (nq, codes) in enumerate(streams):
        got = torch.cat(outs[k]).numpy()
        assert got.dtype == np.float32 and np.array_equal(got, toy_decode(codes.numpy())), k
    assert all(c["B"] <= 3 and c["T"] == HL + block + HR for c in calls) and any(c["B"] > 1 for c in calls)
    per_ring = {}
    for c in calls:
        for r in c["rows"]:
            per_ring.setdefault(r["ring"], []).append(r["start"] + r["emit_lo"])
    assert len(per_ring) == 3                                                        # five sessions, three slots: reuse
    assert sorted(pool._free) == [0, 1, 2] and not pool._sessions


def test_capacity_groups_keep_session_order(pools):
    P, calls = pools
    pool = P.DecodePool(ToyCodec(), capacity=2, block_frames=1)
    rng = np.random.default_rng(3)
    a, b = pool.open(1), pool.open(1)
    ca, cb = (torch.from_numpy(rng.integers(0, 1000, size=(1, 6))) for _ in range(2))
    pool.push(a, ca)
    pool.push(b, cb)                       # ring of 6 frames: 4 windows each are ready at once
    got = pool.step()
    assert [c["B"] for c in calls] == [2, 2, 2, 2] and pool.native_calls == 4 and pool.rows_run == 8
    slot_of = {pool._rings[pool._sessions[s].slot].data_ptr(): s for s in (a, b)}
    order = [(slot_of[r["ring"]], r["start"] + r["emit_lo"]) for c in calls for r in c["rows"]]
    assert order == [(a, 0), (a, 1), (a, 2), (a, 3), (b, 0), (b, 1), (b, 2), (b, 3)]
    assert np.array_equal(torch.cat([got[a], pool.flush(a)]).numpy(), toy_decode(ca.numpy()))
    assert np.array_equal(torch.cat([got[b], pool.flush(b)]).numpy(), toy_decode(cb.numpy()))


@pytest.mark.parametrize("block", [1, 3])
def test_encode_pool_on_the_toy(pools, block):
    """Samples in, codes out: totals that are no multiple of the hop (flush pads), shorter than a block, empty; per-session nq with the
    call's n_quantizers the largest among its rows."""
    P, calls = pools
    rng, nprng = random.Random(block), np.random.default_rng(block)
    pool = P.EncodePool(ToyCodec(), capacity=3, block_frames=block)
    assert pool.ring_cap == (HL + 2 * block + HR - 1) * HOP and pool.delay_samples == (block + HR - 1) * HOP
    streams = [(nq, torch.from_numpy(nprng.integers(-9, 10, size=n).astype(np.float32))) for nq, n in ((4, 61 * HOP + 5), (2, 3), (None, 0), (1, 20 * HOP))]
    sids = [pool.open(nq) for nq, _ in streams[:3]]
    live = {sid: [k, cut(rng, streams[k][1].numel(), [0, 1, 3, HOP - 1, HOP, HOP + 1, 5 * HOP, 30 * HOP]), 0] for k, sid in enumerate(sids)}
    outs = {k: [] for k in range(4)}
    opened_last = False
    while live:
        for sid in list(live):
            k, cuts, pos = live[sid]
            n = cuts.pop(0)
            pool.push(sid, streams[k][1][pos:pos + n])
            live[sid][2] = pos + n
        for sid, y in pool.step().items():
            assert y.dtype == torch.int64
            outs[live[sid][0]].append(y)
        for sid in [s for s in live if not live[s][1]]:
            k = live.pop(sid)[0]
            outs[k].append(pool.flush(sid))
            with pytest.raises(RuntimeError, match="flush"):
                pool.push(sid, torch.zeros(1))
            if not opened_last:                                                       # the fourth session takes a freed slot
                opened_last = True
                sid4 = pool.open(1)
                live[sid4] = [3, cut(rng, streams[3][1].numel(), [HOP, 7 * HOP]), 0]
    for k, (nq, x) in enumerate(streams):
        nq = NCB if nq is None else nq
        pad = (-x.numel()) % HOP
        want = toy_encode(np.concatenate([x.numpy(), np.zeros(pad, np.float32)]), nq) if x.numel() else np.zeros((nq, 0), np.int64)
        got = torch.cat(outs[k], dim=1).numpy()
        assert got.shape == want.shape and np.array_equal(got, want), k
    assert all(c["nq"] == max(r["nq"] for r in c["rows"]) for c in calls)
    assert any(len({r["nq"] for r in c["rows"]}) > 1 for c in calls)                 # sessions with different nq did share calls
    assert all(c["T"] == HL + block + HR for c in calls)


def test_refusals_touch_nothing(pools, monkeypatch):
    P, calls = pools
    dac = ToyCodec()
    for cls in (P.DecodePool, P.EncodePool):
        with pytest.raises(ValueError, match="capacity"):
            cls(dac, capacity=0)
        with pytest.raises(ValueError, match="block_frames"):
            cls(dac, block_frames=0)
        pool = cls(dac, capacity=1)
        for bad in (0, NCB + 1):
            with pytest.raises(RuntimeError, match="codebooks"):
                pool.open(bad)
        sid = pool.open(2)
        with pytest.raises(RuntimeError, match="sessions are open"):
            pool.open(2)
        with pytest.raises(KeyError):
            pool.push(sid + 5, torch.zeros(2, 1, dtype=torch.int64))
        pool.end(sid)
        with pytest.raises(RuntimeError, match="push after flush"):
            pool.push(sid, torch.zeros(2, 1, dtype=torch.int64) if cls is P.DecodePool else torch.zeros(3))
        assert pool.flush(sid).shape == ((0,) if cls is P.DecodePool else (2, 0))
        with pytest.raises(RuntimeError, match="flushed"):
            pool.flush(sid)
        assert pool.open(1) == sid + 1                                               # the slot is free again
    pool = P.DecodePool(dac, capacity=1)
    sid = pool.open(2)
    with pytest.raises(RuntimeError, match="code rows"):
        pool.push(sid, torch.zeros(3, 1, dtype=torch.int64))
    with pytest.raises(TypeError):
        pool.push(sid, torch.zeros(2, 1))
    enc = P.EncodePool(dac)
    for bad in (torch.zeros(4, dtype=torch.float64), torch.zeros(2, 2)):
        with pytest.raises(TypeError):
            enc.push(enc.open(), bad)
    odd = ToyCodec()
    odd.decoder_rates = (4, 5)
    with pytest.raises(RuntimeError, match="decoder rate 5 is odd"):
        P.DecodePool(odd)
    assert not calls
    monkeypatch.undo()                                                               # the real device check: a codec on the CPU
    from flowdec_amd import ndac_pool
    for cls in (ndac_pool.DecodePool, ndac_pool.EncodePool):
        with pytest.raises(RuntimeError, match="must be on the GPU"):
            cls(dac)


def test_symbols_and_struct_layout():
    import re, os
    from flowdec_amd import _lib
    from flowdec_amd import build
    lib = _lib.load()
    src = open(os.path.join(os.path.dirname(build.HERE), "include", "flowdec_hip.h")).read()
    decl = set(re.findall(r"\b(fd_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", src, flags=re.S)))
    for name in ("fd_ndac_pool_workspace_bytes", "fd_ndac_pool_decode", "fd_ndac_pool_encode"):
        assert name in decl and name in _lib.SIGNATURES and getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
    assert "ndac_pool.hip" in build.SOURCES
    assert C.sizeof(_lib.FdNdacPoolRow) == 48
    assert [getattr(_lib.FdNdacPoolRow, f).offset for f, _ in _lib.FdNdacPoolRow._fields_] == [0, 8, 16, 20, 24, 28, 32, 40]
    one = C.c_void_p(8)
    assert lib.fd_ndac_pool_decode(None, one, one, 1, 4, one, 1 << 20, 0, None) != 0     # no codec: refused on the host
    assert lib.fd_ndac_pool_encode(None, one, one, 1, 4, 1, one, 1 << 20, 0, None) != 0
    assert lib.fd_ndac_pool_workspace_bytes(None, 1, 4) == 0
