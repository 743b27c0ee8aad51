"""Streaming enhance on the GPU (include/flowdec_hip.h "Streaming"; flowdec_amd/stream.py; flowdec_amd/stream_cli.py).

The two device steps against NumPy restatements, exactly; then the contract: what a session returns, concatenated, is `enhance_long` on
the concatenated input bit for bit -- however the input was cut into pushes, whichever other sessions shared its native calls.  Geometry
and model as tests/test_hip_longform.py: nf = 8, rows of 64 frames, halos of 8, N = 2, euler."""
import numpy as np
import pytest
import torch

from test_hip_longform import HALO, HOP, N3, N4, RF, STRIDE, W, X, _file, _flow, _plan

pytestmark = pytest.mark.gpu

KW = dict(N=2, solver="euler", row_frames=RF, halo_frames=HALO)
LENGTHS = {"W": W, "W+1": W + 1, "S+W": STRIDE + W, "N3": N3, "N4": N4}
_refs = {}


def _table(entries):
    """[dict of fd_stream_row fields] -> the device table (uint8)."""
    from flowdec_amd import _lib as L
    rows = (L.FdStreamRow * len(entries))()
    for e, d in zip(rows, entries):
        for k, v in d.items():
            setattr(e, k, v)
    return torch.from_numpy(np.frombuffer(bytes(rows), dtype=np.uint8).copy()).cuda()


def _gather(entries, Lrow, peak=None):
    from flowdec_amd import _lib as L
    t = _table(entries)
    y = torch.full((len(entries), Lrow), float("nan"), device="cuda")
    nf = torch.full((len(entries),), float("nan"), device="cuda") if peak is not None else None
    L.check(L.load().fd_stream_gather(L.ptr(t), len(entries), L.ptr(y), Lrow, L.ptr(peak), L.ptr(nf), L.stream()))
    torch.cuda.synchronize()
    return y.cpu().numpy(), None if nf is None else nf.cpu().numpy()


def _gather_ref(rings, entries, Lrow):
    y = np.zeros((len(entries), Lrow), dtype=np.float32)
    for b, (ring, e) in enumerate(zip(rings, entries)):
        idx = (e["start"] + np.arange(e["length"], dtype=np.int64)) % e["ring_cap"]
        y[b, :e["length"]] = ring[idx]
    return y


# ---- 1. fd_stream_gather -----------------------------------------------------------------------------------------------------------
def test_gather_equals_numpy_wrapped_ring_and_zero_tail():
    rng = np.random.default_rng(0)
    for cap, Lrow in ((1003, 777), (4099, 2500)):                    # no multiples of the workgroup; 2500: several strides per thread
        host = [rng.standard_normal(cap).astype(np.float32) for _ in range(2)]
        dev = [torch.from_numpy(h).cuda() for h in host]
        spec = [(0, 5 * cap + cap - 100, Lrow - 77),                  # wraps; a zero tail of 77
                (1, 17, Lrow),                                        # the full row
                (0, 2 ** 33 + 5, 1),                                  # ONE sample, an absolute index beyond 32 bits
                (1, 3 * cap - 1, min(cap, Lrow))]                     # starts on the ring's last element
        entries = [dict(ring=dev[r].data_ptr(), start=s, ring_cap=cap, length=n, peak_slot=0) for r, s, n in spec]
        got, _ = _gather(entries, Lrow)
        assert np.array_equal(got, _gather_ref([host[r] for r, _, _ in spec], entries, Lrow)), (cap, Lrow)


def test_gather_peak_carry_and_guard():
    rng = np.random.default_rng(1)
    cap, Lrow = 2048, 1500
    host = rng.uniform(-0.5, 0.5, (4, cap)).astype(np.float32)
    host[0, 700] = -0.75                                             # row 0's own peak, negative
    host[1] = 0.0                                                    # silence: 1
    host[2] *= np.float32(1e-8)                                      # max <= 1e-8: 1
    host[3, 2047] = 0.9                                              # outside the row below: not counted
    dev = torch.from_numpy(host).cuda()
    entries = [dict(ring=dev[b].data_ptr(), start=cap * 7, ring_cap=cap, length=Lrow - b, peak_slot=(3, 0, 2, 5)[b]) for b in range(4)]
    peak0 = np.array([0.0, 9.0, 0.0, 0.25, 9.0, 2.5], dtype=np.float32)            # slots 1 and 4 belong to nobody
    peak = torch.from_numpy(peak0.copy()).cuda()
    got, nf = _gather(entries, Lrow, peak)
    rows = _gather_ref(host, entries, Lrow)
    assert np.array_equal(got, rows)
    own = np.abs(rows).max(axis=1)
    assert own[0] == np.float32(0.75) and own[1] == 0 and 0 < own[2] <= 1e-8 and own[3] <= 0.5
    want_peak = peak0.copy()
    for b, e in enumerate(entries):
        want_peak[e["peak_slot"]] = max(peak0[e["peak_slot"]], own[b])
    assert np.array_equal(peak.cpu().numpy(), want_peak)
    assert np.array_equal(nf, np.array([0.75, 1.0, 1.0, 2.5], dtype=np.float32))   # own peak; silence; the guard; the carried peak
    assert peak.cpu().numpy()[2] == own[2]                                         # the guard is on the factor, not on the carry
    # the carry across calls: a quieter row after a louder one keeps the factor, a louder one raises it
    host2 = rng.uniform(-0.3, 0.3, cap).astype(np.float32)
    dev2 = torch.from_numpy(host2).cuda()
    _, nf = _gather([dict(ring=dev2.data_ptr(), start=0, ring_cap=cap, length=Lrow, peak_slot=3)], Lrow, peak)
    assert nf[0] == np.float32(0.75)
    host2[5] = 0.8
    dev2.copy_(torch.from_numpy(host2))
    _, nf = _gather([dict(ring=dev2.data_ptr(), start=0, ring_cap=cap, length=Lrow, peak_slot=3)], Lrow, peak)
    assert nf[0] == np.float32(0.8) and peak.cpu().numpy()[3] == np.float32(0.8)


def test_gather_int16_origin():
    rng = np.random.default_rng(2)
    cap, Lrow = 1536, 1200
    pcm = rng.integers(-20000, 20000, cap).astype(np.int16)
    pcm[100], pcm[1300] = -32768, 32767
    ring = (torch.from_numpy(pcm).cuda().to(torch.float32) * (1.0 / 32768.0))      # push()'s conversion
    host = pcm.astype(np.float32) / np.float32(32768)
    assert np.array_equal(ring.cpu().numpy(), host) and np.array_equal(host.astype(np.float64) * 32768, pcm)    # exact
    peak = torch.zeros(2, device="cuda")
    entries = [dict(ring=ring.data_ptr(), start=1000, ring_cap=cap, length=Lrow, peak_slot=0),      # holds -32768 (wrapped) -> 1.0
               dict(ring=ring.data_ptr(), start=200, ring_cap=cap, length=1000, peak_slot=1)]
    got, nf = _gather(entries, Lrow, peak)
    want = _gather_ref([host, host], entries, Lrow)
    assert np.array_equal(got, want)
    assert nf[0] == 1.0 and nf[1] == np.abs(want[1]).max() and float(nf[1]) * 32768 == int(np.abs(pcm[200:1200].astype(np.int32)).max())


# ---- 2. fd_stream_emit ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("xfade", [X, 2, 0])
def test_emit_equals_numpy_float32_three_rows_two_sessions(xfade):
    """Session A: the 4 rows of N4, session B: the 3 rows of N3 -- unrelated random rows, so every weight matters.  Launch k carries row k of
    both (the fourth: A alone); the tails go through two buffers per session by row parity.  Concatenated == stitch_reference, exactly."""
    from flowdec_amd import _lib as L
    from flowdec_amd.longform import StreamPlanner, stitch_reference, stitch_weights
    rng = np.random.default_rng(3 + xfade)
    half = xfade // 2
    w = torch.from_numpy(stitch_weights(xfade)).cuda() if xfade else None
    sess = []
    for n in (N4, N3):
        p = StreamPlanner(HOP, RF, HALO, xfade)
        p.push(n)
        srs = []
        while p.ready():
            srs.append(p.next_row())
        srs.append(p.flush())
        assert [s.row for s in srs] == _plan(n, xfade)
        outs = [rng.standard_normal(s.row.length).astype(np.float32) for s in srs]
        sess.append(dict(n=n, srs=srs, outs=outs, want=stitch_reference(outs, [s.row for s in srs], xfade),
                         tails=torch.full((2, max(xfade, 1)), float("nan"), device="cuda"), got=[]))
    assert len(sess[0]["srs"]) == 4 and len(sess[1]["srs"]) == 3
    for k in range(4):
        live = [s for s in sess if k < len(s["srs"])]
        B = len(live)
        x_hat = torch.full((B, W), float("nan"), device="cuda")
        fin = torch.full((B, W), float("nan"), device="cuda")
        entries = []
        for b, s in enumerate(live):
            sr = s["srs"][k]
            x_hat[b, :sr.row.length] = torch.from_numpy(s["outs"][k])
            entries.append(dict(emit_lo=sr.finished[0] - sr.row.start, emit_count=sr.finished[1] - sr.finished[0],
                                tail_lo=0 if sr.last else sr.row.xfade_hi - half - sr.row.start,
                                tail_in=s["tails"][(k - 1) % 2].data_ptr() if xfade and k > 0 else None,
                                tail_out=s["tails"][k % 2].data_ptr() if xfade and not sr.last else None, out=fin[b].data_ptr()))
        t = _table(entries)
        L.check(L.load().fd_stream_emit(L.ptr(t), B, L.ptr(x_hat), W, L.ptr(w), xfade, L.stream()))
        torch.cuda.synchronize()
        for b, s in enumerate(live):
            sr = s["srs"][k]
            cnt = sr.finished[1] - sr.finished[0]
            s["got"].append(fin[b, :cnt].cpu().numpy())
            assert torch.isnan(fin[b, cnt:]).all()                                  # nothing written beyond the finished range
            if xfade and not sr.last:                                               # the tail handed over = this row around its upper boundary
                lo = sr.row.xfade_hi - half - sr.row.start
                assert np.array_equal(s["tails"][k % 2].cpu().numpy(), s["outs"][k][lo:lo + xfade])
    for s in sess:
        got = np.concatenate(s["got"])
        assert got.shape == (s["n"],) and np.array_equal(got, s["want"]), s["n"]


# ---- 3. one stream == enhance_long ---------------------------------------------------------------------------------------------------
def _late_peak_file(n, seed):
    """Peaks planted late: the rows' causal factors differ (0.5-clipped noise, then 0.7 past the middle, then 0.9 in the LAST sample: beyond every row but the last)."""
    y = _file(n, seed=seed)
    y[int(0.55 * n)] = 0.7
    y[n - 1] = -0.9
    return y


def _reference(precision, nf_kind, name):
    """enhance_long on the whole file, once per (precision, normalisation, length)."""
    key = (precision, nf_kind, name)
    if key not in _refs:
        n = LENGTHS[name]
        y = _late_peak_file(n, seed=n % 97)
        normfac = 0.7 if nf_kind == "fixed" else "causal"
        ref = _flow(precision).enhance_long(torch.from_numpy(y), seed=31, normfac=normfac, **KW)
        assert ref.shape == (n,) and torch.isfinite(ref).all() and ref.abs().max() > 0
        _refs[key] = (y, normfac, ref)
    return _refs[key]


def _cut(n, pattern, rng):
    if pattern == "one":
        return [n]
    if pattern == "997":
        return [997] * (n // 997) + ([n % 997] if n % 997 else [])
    sizes, left = [], n
    while left:
        k = min(left, int(rng.integers(1, 30000)))
        sizes.append(k)
        left -= k
    return sizes


def _stream(m, y, sizes, seed, normfac, **kw):
    from flowdec_amd.stream import EnhanceStream
    st = EnhanceStream(m, seed=seed, normfac=normfac, **dict(KW, **kw))
    outs, pos = [], 0
    for k in sizes:
        outs.append(st.push(y[pos:pos + k]))
        pos += k
    outs.append(st.flush())
    return torch.cat(outs).cpu(), st.pool


@pytest.mark.parametrize("name", list(LENGTHS))
@pytest.mark.parametrize("nf_kind", ["fixed", "causal"])
@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_stream_equals_enhance_long(precision, nf_kind, name):
    m = _flow(precision)
    y, normfac, ref = _reference(precision, nf_kind, name)
    n = len(y)
    rows = _plan(n)
    if nf_kind == "causal" and len(rows) > 1:                       # the rows' factors do differ
        assert len({float(np.abs(y[:r.start + r.length]).max()) for r in rows}) > 1
    rng = np.random.default_rng(n)
    for pattern in ("one", "997", "random"):
        got, pool = _stream(m, torch.from_numpy(y), _cut(n, pattern, rng), 31, normfac)
        assert got.shape == ref.shape and torch.equal(got, ref), (pattern, float((got - ref).abs().max()))
        assert pool.rows_run == pool.native_calls == len(rows)


def test_causal_is_not_the_file_maximum_and_fixed_is_not_causal():
    """The references above are three different normalisations (otherwise the tests above would not tell them apart)."""
    m = _flow("bf16")
    y, _, causal = _reference("bf16", "causal", "N3")
    _, _, fixed = _reference("bf16", "fixed", "N3")
    whole = m.enhance_long(torch.from_numpy(y), seed=31, **KW)
    assert not torch.equal(causal, whole) and not torch.equal(fixed, whole) and not torch.equal(causal, fixed)
    assert torch.equal(m.enhance_long(torch.from_numpy(y), seed=31, normfac=0.9, **KW), whole)       # 0.9 IS the file's maximum
    assert torch.equal(m.enhance_long(torch.from_numpy(y), seed=31, normfac=torch.tensor([0.7]), **KW), fixed)
    # enhance_long_rows takes the same option; its stitch is enhance_long
    rows = m.enhance_long_rows(torch.from_numpy(y), seed=31, normfac="causal", **KW)
    assert torch.equal(m.enhance_long_stitch(torch.from_numpy(y), rows, row_frames=RF, halo_frames=HALO), causal)
    with pytest.raises(ValueError):
        m.enhance_long(torch.from_numpy(y), seed=31, normfac="peak", **KW)
    with pytest.raises(ValueError):
        _flow("bf16", "none").enhance_long(torch.from_numpy(y), seed=31, normfac=0.7, **KW)


def test_enhance_long_without_normfac_is_unchanged():
    """normfac=None is the two-halves path, bit for bit."""
    m = _flow("bf16")
    y = torch.from_numpy(_file(N4, seed=41))
    whole = m.enhance_long(y, seed=5, **KW)
    rows = m.enhance_long_rows(y, seed=5, **KW)
    assert torch.equal(whole, m.enhance_long_stitch(y, rows, row_frames=RF, halo_frames=HALO))
    assert torch.equal(whole, m.enhance_long(y, seed=5, normfac=None, **KW))


def test_none_model_and_device_pushes():
    """normalize_mode='none': no factor at all; pushes from device memory; a buffer the caller reuses between pushes."""
    from flowdec_amd.stream import EnhanceStream
    m = _flow("bf16", "none")
    y = torch.from_numpy(_file(N3, seed=42))
    ref = m.enhance_long(y, seed=6, **KW)
    st = EnhanceStream(m, seed=6, normfac=None, **KW)
    buf = torch.empty(50000)
    outs, pos = [], 0
    while pos < N3:
        k = min(50000, N3 - pos)
        buf[:k] = y[pos:pos + k]                                    # 50000 > what the ring takes at once: part of it waits on the host
        outs.append(st.push(buf[:k].cuda() if pos else buf[:k]))
        pos += k
    outs.append(st.flush())
    assert all(o.is_cuda for o in outs) and torch.equal(torch.cat(outs).cpu(), ref)


def test_recording_inside_its_first_row_runs_in_its_own_bucket():
    """Rows of 128 frames: a recording of 20000 samples is ONE row, which enhance_long runs in the 64-frame bucket of its own length (it is
    `enhance(seed=)`); one of 130 frames' worth runs in the row's bucket; a two-row recording at this geometry for good measure."""
    m = _flow("bf16")
    kw = dict(row_frames=128, halo_frames=32)
    for n in (20000, 80 * HOP, 128 * HOP + 5):
        y = torch.from_numpy(_late_peak_file(n, seed=44))
        got, pool = _stream(m, y, _cut(n, "997", None), 9, "causal", **kw)
        assert torch.equal(got, m.enhance_long(y, seed=9, normfac="causal", **dict(KW, **kw))), n
        assert pool.native_calls == (2 if n > 128 * HOP else 1)
    assert torch.equal(_stream(m, y[:20000], [20000], 9, "causal", **kw)[0], m.enhance(y[:20000], N=2, solver="euler", seed=9))


def test_int16_push_equals_float_push():
    m = _flow("bf16")
    n = STRIDE + W
    pcm = torch.from_numpy(np.clip(np.rint(_late_peak_file(n, seed=43) * 32768), -32768, 32767).astype(np.int16))
    as_float = pcm.to(torch.float32) / 32768
    sizes = _cut(n, "random", np.random.default_rng(4))
    a, _ = _stream(m, pcm, sizes, 8, "causal")
    b, _ = _stream(m, as_float, [n], 8, "causal")
    assert torch.equal(a, b) and torch.isfinite(a).all() and a.abs().max() > 0
    assert torch.equal(a, m.enhance_long(as_float, seed=8, normfac="causal", **KW))


# ---- 4. the pool -------------------------------------------------------------------------------------------------------------------------
def test_pool_sessions_equal_their_solo_results():
    """Three sessions of different lengths, seeds and push schedules in one pool (capacity 4): each equals its solo stream and enhance_long."""
    from flowdec_amd.stream import StreamPool
    m = _flow("bf16")
    spec = [(W + 1, 101, 4097), (N3, (1 << 63) + 102, 5000), (N4, 103, 4801)]      # (samples, seed, block): rows 0 of sessions 0 and 2 meet in round 6
    ys = [torch.from_numpy(_late_peak_file(n, seed=50 + i)) for i, (n, _, _) in enumerate(spec)]
    pool = StreamPool(m, capacity=4, normfac="causal", **KW)
    sids = [pool.open([seed]) for _, seed, _ in spec]
    outs = {sid: [] for sid in sids}
    pos = [0, 0, 0]
    shared = 0
    while any(p < n for p, (n, _, _) in zip(pos, spec)):
        for i, (n, _, block) in enumerate(spec):
            if pos[i] < n:
                k = min(n - pos[i], block)
                pool.push(sids[i], ys[i][pos[i]:pos[i] + k])
                pos[i] += k
        got = pool.step()
        shared += len(got) > 1
        for sid, o in got.items():
            outs[sid].append(o)
    while True:                                                       # what the host queues still hold
        got = pool.step()
        if not got:
            break
        for sid, o in got.items():
            outs[sid].append(o)
    for sid in sids:
        outs[sid].append(pool.flush(sid))
    assert shared >= 1, "no native call carried two sessions: the test shows nothing"
    assert pool.rows_run == 2 + 3 + 4 and pool.native_calls < pool.rows_run
    for i, (n, seed, _) in enumerate(spec):
        got = torch.cat(outs[sids[i]]).cpu()
        solo, _ = _stream(m, ys[i], [n], [seed], "causal")
        assert torch.equal(got, solo), f"session {i} != its solo stream"
        assert torch.equal(got, m.enhance_long(ys[i], seed=[seed], normfac="causal", **KW)), f"session {i} != enhance_long"
    with pytest.raises(KeyError):
        pool.push(sids[0], ys[0][:10])                                # flushed sessions are closed, their slots free again
    assert len([pool.open(1) for _ in range(4)]) == 4
    with pytest.raises(RuntimeError):
        pool.open(2)


def test_pool_in_lockstep_shares_every_call():
    """Three sessions of one length pushed in lockstep: native_calls == the rows of ONE session."""
    from flowdec_amd.stream import StreamPool
    m = _flow("bf16")
    ys = [torch.from_numpy(_late_peak_file(N3, seed=60 + i)) for i in range(3)]
    pool = StreamPool(m, capacity=3, normfac=0.7, **KW)
    sids = [pool.open(200 + i) for i in range(3)]
    outs = {sid: [] for sid in sids}
    for pos in range(0, N3, 7001):
        for sid, y in zip(sids, ys):
            pool.push(sid, y[pos:pos + 7001])
        for sid, o in pool.step().items():
            outs[sid].append(o)
    assert not pool.step()
    for sid, o in pool.flush_many(sids).items():
        outs[sid].append(o)
    assert pool.native_calls == len(_plan(N3)) == 3 and pool.rows_run == 9
    for i, (sid, y) in enumerate(zip(sids, ys)):
        assert torch.equal(torch.cat(outs[sid]).cpu(), m.enhance_long(y, seed=200 + i, normfac=0.7, **KW)), i


# ---- 5. the command line -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["f32le", "s16le"])
def test_stream_cli_reproduces_the_api(tmp_path, fmt):
    from test_cli import synthetic_ckpt
    from flowdec_amd import enhance_cli, stream_cli
    torch.save(synthetic_ckpt(), tmp_path / "m.ckpt")
    n = STRIDE + W + 123
    y = _late_peak_file(n, seed=70)
    if fmt == "s16le":
        pcm = np.clip(np.rint(y * 32768), -32768, 32767).astype("<i2")
        pcm.tofile(tmp_path / "in.raw")
        y = pcm.astype(np.float32) / np.float32(32768)
    else:
        y.astype("<f4").tofile(tmp_path / "in.raw")
    written = stream_cli.run(["--ckpt", str(tmp_path / "m.ckpt"), "--N", "2", "--solver", "euler", "--seed", "7", "--row-frames", str(RF),
                              "--halo-frames", str(HALO), "--normfac", "causal", "--format", fmt, "--in", str(tmp_path / "in.raw"),
                              "--out", str(tmp_path / "out.raw"), "--block-samples", "4801"])
    m = enhance_cli.load_from_checkpoint(str(tmp_path / "m.ckpt"), map_location="cuda:0", model="flow")
    want = m.enhance_long(torch.from_numpy(y), seed=7, normfac="causal", **KW)
    assert written == n and torch.isfinite(want).all() and want.abs().max() > 0
    assert (tmp_path / "out.raw").read_bytes() == stream_cli.encode(want, fmt)
    if fmt == "f32le":
        assert np.array_equal(np.fromfile(tmp_path / "out.raw", dtype="<f4"), want.numpy())
