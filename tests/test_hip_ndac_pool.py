"""Codec session pools on the GPU (include/flowdec_hip.h "Codec pools"; csrc/ndac_pool.hip; flowdec_amd/ndac_pool.py).

Every comparison is bit equality against the one-shot `DAC.decode` / `DAC.encode` (the references of tests/test_hip_ndac_stream.py and
tests/test_hip_ndac_encode_stream.py, computed once and shared), never against the pool itself: a session's concatenated output is its
one-shot result however its input was cut, whichever sessions shared its calls, with or without the graph.
Builds: NDAC75_LIKE (vector path), WIDE_DECODER / WIDE_ENCODER (matrix-core layers run)."""
import random

import pytest
import torch

import test_hip_ndac_encode_stream as ES
import test_hip_ndac_stream as DS

pytestmark = pytest.mark.gpu

DEC_BUILDS = [("ndac75", "exact"), ("ndac75", "mfma_decoder"), ("wide", "exact"), ("wide", "mfma_decoder")]
ENC_BUILDS = [("ndac75", "exact"), ("wide", "mfma")]


def drain(pool, outs):
    """Steps until nothing is ready; appends to outs[sid]."""
    while True:
        got = pool.step()
        if not got:
            return
        for sid, y in got.items():
            outs.setdefault(sid, []).append(y)


def feed(pool, sid, data, sizes, outs, step=True):
    """Pushes `data` (last axis) in pieces of `sizes`, stepping after each."""
    pos = 0
    for n in sizes:
        pool.push(sid, data[..., pos:pos + n])
        pos += n
        if step:
            drain(pool, outs)
    assert pos == data.shape[-1]


def joined(outs, sid, tail):
    return torch.cat(outs.get(sid, []) + [tail], dim=-1)


# ---- decode ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,precision", DEC_BUILDS)
def test_mixed_phases_share_one_call(name, precision):
    """A first window (11 frames, true left edge), a mid-stream window (20 frames) and the last window of a one-frame stream (a 1-frame
    emit) as the three rows of ONE native call."""
    from flowdec_amd.ndac_pool import DecodePool
    m = DS.model(name, precision)
    assert m.decode_halo() == (9, 9)
    nq = 4
    (ca, wa), (cb, wb), (cc, wc) = DS.one_shot(name, precision, nq, 14, 2), DS.one_shot(name, precision, nq, 30, 3), DS.one_shot(name, precision, nq, 1, 4)
    pool = DecodePool(m, capacity=5, block_frames=2, use_graph=False)
    assert (pool.T, pool.ring_cap, pool.delay_samples) == (20, 21, 10 * m.hop_length)
    a, b, c = pool.open(nq), pool.open(nq), pool.open(nq)
    outs = {}
    pool.push(b, cb[:, :19])                       # frames [0, 10) leave: five windows, one call
    drain(pool, outs)
    assert (pool.native_calls, pool.rows_run) == (1, 5)
    pool.push(a, ca[:, :11])
    pool.push(b, cb[:, 19:21].cuda())              # (a device push)
    pool.push(c, cc)
    pool.end(c)
    got = pool.step()
    assert (pool.native_calls, pool.rows_run) == (2, 8) and set(got) == {a, b, c}
    hop = m.hop_length
    assert got[a].shape == (2 * hop,) and got[b].shape == (2 * hop,) and got[c].shape == (hop,)
    assert torch.equal(got[c], wc)
    assert torch.equal(got[a], wa[:2 * hop]) and torch.equal(got[b], wb[10 * hop:12 * hop])
    outs.setdefault(a, []).append(got[a])
    outs[b].append(got[b])
    pool.push(a, ca[:, 11:])
    pool.push(b, cb[:, 21:])
    drain(pool, outs)
    assert torch.equal(joined(outs, a, pool.flush(a)), wa) and torch.equal(joined(outs, b, pool.flush(b)), wb)
    assert not pool._sessions and sorted(pool._free) == list(range(5))


@pytest.mark.parametrize("name,precision", [("ndac75", "exact"), ("wide", "mfma_decoder")])
def test_ring_wraps_under_random_cuts(name, precision):
    """75 frames through a ring of 21: it wraps three times; empty pushes and one push that completes several blocks at once."""
    from flowdec_amd.ndac_pool import DecodePool
    m = DS.model(name, precision)
    codes, want = DS.one_shot(name, precision, 4, 75, 5)
    rng = random.Random(7)
    sizes = DS.cut(rng, 75 - 13)
    sizes.insert(len(sizes) // 2, 13)
    assert 0 in sizes
    pool = DecodePool(m, capacity=4, block_frames=2, use_graph=False)
    sid, outs = pool.open(4), {}
    feed(pool, sid, codes, sizes, outs)
    got = joined(outs, sid, pool.flush(sid))
    assert torch.equal(got, want)
    assert pool.rows_run == 34 and pool.native_calls < pool.rows_run            # 33 blocks and the rest; some calls carried several rows


def test_sessions_with_different_nq_share_every_call():
    from flowdec_amd.ndac_pool import DecodePool
    name, precision = "wide", "mfma_decoder"
    m = DS.model(name, precision)
    (c2, w2), (c4, w4) = DS.one_shot(name, precision, 2, 30, 3), DS.one_shot(name, precision, 4, 30, 3)
    pool = DecodePool(m, capacity=2, block_frames=3, use_graph=False)
    s2, s4 = pool.open(2), pool.open(4)
    outs = {}
    for p in range(0, 30, 3):
        pool.push(s2, c2[:, p:p + 3])
        pool.push(s4, c4[:, p:p + 3])
        drain(pool, outs)
    pool.end(s2)
    pool.end(s4)
    drain(pool, outs)
    assert pool.rows_run == 2 * pool.native_calls and not pool._sessions
    assert torch.equal(torch.cat(outs[s2]), w2) and torch.equal(torch.cat(outs[s4]), w4)
    assert not torch.equal(w2, w4)


def test_alone_or_in_company_and_slots_reused():
    """A session alone in a pool of one slot and the same session among four others in a pool of three slots (five sessions over time:
    slots are reused after flush): the same bits, the one-shot decode's."""
    from flowdec_amd.ndac_pool import DecodePool
    name, precision = "ndac75", "mfma_decoder"
    m = DS.model(name, precision)
    codes, want = DS.one_shot(name, precision, 4, 30, 3)
    solo = DecodePool(m, capacity=1, block_frames=2, use_graph=False)
    sid, outs = solo.open(4), {}
    feed(solo, sid, codes, [7, 0, 11, 12], outs)
    alone = joined(outs, sid, solo.flush(sid))
    pool = DecodePool(m, capacity=3, block_frames=2, use_graph=False)
    others = [DS.one_shot(name, precision, nq, T, seed) for nq, T, seed in ((4, 14, 2), (4, 1, 4), (4, 75, 5), (10, 12, 6))]
    outs, done = {}, {}
    o0, o1 = pool.open(4), pool.open(4)
    pool.push(o0, others[0][0])
    pool.push(o1, others[1][0])
    drain(pool, outs)
    done[0], done[1] = joined(outs, o0, pool.flush(o0)), joined(outs, o1, pool.flush(o1))     # two slots free again
    o2, x, o3 = pool.open(4), pool.open(4), pool.open(10)
    used = {pool._sessions[s].slot for s in (o2, x, o3)}
    assert used == {0, 1, 2}
    with pytest.raises(RuntimeError, match="sessions are open"):
        pool.open(4)
    for p in range(0, 75, 5):
        pool.push(o2, others[2][0][:, p:p + 5])
        pool.push(x, codes[:, 2 * (p // 5):2 * (p // 5) + 2])
        pool.push(o3, others[3][0][:, p:p + 5])
        drain(pool, outs)
    done[2], in_company, done[3] = joined(outs, o2, pool.flush(o2)), joined(outs, x, pool.flush(x)), joined(outs, o3, pool.flush(o3))
    assert torch.equal(alone, want) and torch.equal(in_company, alone)
    for k in range(4):
        assert torch.equal(done[k], others[k][1]), k
    assert pool.rows_run > pool.native_calls


@pytest.mark.parametrize("name,precision", [("ndac75", "exact"), ("wide", "mfma_decoder")])
def test_graph_equals_eager_and_pools_do_not_disturb_each_other(name, precision):
    """A whole stream -- short first windows, full windows, the short last one -- through the captured step; a second pool on the same
    codec runs between its steps."""
    from flowdec_amd.ndac_pool import DecodePool
    m = DS.model(name, precision)
    codes, want = DS.one_shot(name, precision, 4, 30, 3)
    codes2, want2 = DS.one_shot(name, precision, 4, 14, 2)
    res = {}
    for use_graph in (False, True):
        pool, other = DecodePool(m, capacity=2, block_frames=1, use_graph=use_graph), DecodePool(m, capacity=2, block_frames=1, use_graph=use_graph)
        sid, sid2, outs, outs2 = pool.open(4), other.open(4), {}, {}
        for p in range(30):
            pool.push(sid, codes[:, p:p + 1])
            drain(pool, outs)
            if p < 14:
                other.push(sid2, codes2[:, p:p + 1])
                drain(other, outs2)
        res[use_graph] = joined(outs, sid, pool.flush(sid)), joined(outs2, sid2, other.flush(sid2))
        assert pool.native_calls == 22 and other.native_calls == 6          # 30 - 9 blocks + the rest; 14 - 9 + the rest
    assert torch.equal(res[False][0], want) and torch.equal(res[False][1], want2)
    assert torch.equal(res[True][0], want) and torch.equal(res[True][1], want2)


# ---- encode ----------------------------------------------------------------------------------------------------------------------------
def nan_rings(pool):
    """What a window must never read as data: everything in the rings before the first push."""
    pool._rings.fill_(float("nan"))
    return pool


@pytest.mark.parametrize("name,precision", ENC_BUILDS)
def test_encode_mixed_phases_share_one_call(name, precision):
    from flowdec_amd.ndac_pool import EncodePool
    m = ES.model(name, precision)
    assert m.encode_halo() == (7, 7)
    hop, nq = m.hop_length, 3
    (xa, ra), (xb, rb), (xc, rc) = ES.one_shot(name, precision, nq, 12 * hop, 2), ES.one_shot(name, precision, nq, 26 * hop + 17, 3), ES.one_shot(name, precision, nq, 5, 4)
    pool = nan_rings(EncodePool(m, capacity=4, block_frames=2, use_graph=False))
    assert (pool.T, pool.ring_cap, pool.delay_samples) == (16, 17 * hop, 8 * hop)
    a, b, c = pool.open(nq), pool.open(nq), pool.open(nq)
    outs = {}
    pool.push(b, xb[:15 * hop + 3])                # frames [0, 8) leave: four windows, one call
    drain(pool, outs)
    assert (pool.native_calls, pool.rows_run) == (1, 4)
    pool.push(a, xa[:9 * hop])                     # the first window: 9 frames, true left edge
    pool.push(b, xb[15 * hop + 3:17 * hop].cuda())  # the mid-stream window: frames [1, 17), final [8, 10)
    pool.push(c, xc)                               # five samples: one zero-padded frame, the whole stream
    pool.end(c)
    got = pool.step()
    assert (pool.native_calls, pool.rows_run) == (2, 7) and set(got) == {a, b, c}
    assert got[c].dtype == torch.int64 and torch.equal(got[c], rc[1][0]) and got[c].shape == (nq, 1)
    assert torch.equal(got[a], ra[1][0][:, :2]) and torch.equal(got[b], rb[1][0][:, 8:10])
    outs.setdefault(a, []).append(got[a])
    outs[b].append(got[b])
    pool.push(a, xa[9 * hop:])
    pool.push(b, xb[17 * hop:])
    drain(pool, outs)
    assert torch.equal(joined(outs, a, pool.flush(a)), ra[1][0])
    assert torch.equal(joined(outs, b, pool.flush(b)), rb[1][0])                # 26 frames and 17 samples: flush pads the 27th


@pytest.mark.parametrize("name,precision", ENC_BUILDS)
def test_encode_wrap_nq_company_and_reuse(name, precision):
    """The ring wraps under random cuts; sessions with different nq share calls; a session alone equals itself in company; slots are
    reused; totals shorter than a block and no multiple of the hop; the rings start as NaN."""
    from flowdec_amd.ndac_pool import EncodePool
    m = ES.model(name, precision)
    hop = m.hop_length
    x, ref = ES.one_shot(name, precision, 3, 61 * hop + 5, 5)
    want = ref[1][0]
    rng = random.Random(11)
    solo = nan_rings(EncodePool(m, capacity=1, block_frames=2, use_graph=False))
    sid, outs = solo.open(3), {}
    feed(solo, sid, x, ES.cut(rng, x.numel()), outs)
    alone = joined(outs, sid, solo.flush(sid))
    assert torch.equal(alone, want) and solo.rows_run >= 27
    pool = nan_rings(EncodePool(m, capacity=3, block_frames=2, use_graph=True))
    small = [ES.one_shot(name, precision, nq, total, seed) for nq, total, seed in ((1, 5, 4), (None, hop, 6), (2, 3 * hop - 1, 7))]
    outs, done = {}, {}
    s0, s1 = pool.open(1), pool.open(None)
    pool.push(s0, small[0][0])
    pool.push(s1, small[1][0])
    done[0], done[1] = pool.flush(s0), pool.flush(s1)
    s2, sx = pool.open(2), pool.open(3)
    assert {pool._sessions[s].slot for s in (s2, sx)} <= {0, 1, 2} and len(pool._free) == 1
    pool.push(s2, small[2][0])
    pool.end(s2)
    sizes = ES.cut(rng, x.numel())
    pos = 0
    for n in sizes:
        pool.push(sx, x[pos:pos + n])
        pos += n
        drain(pool, outs)
    done[2] = torch.cat(outs[s2], dim=1)
    in_company = joined(outs, sx, pool.flush(sx))
    assert torch.equal(in_company, alone)
    for k, nq in enumerate((1, m.n_codebooks, 2)):
        assert done[k].shape[0] == nq and torch.equal(done[k], small[k][1][1][0]), k
    assert all(bool(torch.isfinite(t.float()).all()) for t in (alone, in_company))


# ---- the host table's checks -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("encode", [False, True], ids=["decode", "encode"])
def test_bad_tables_are_refused_before_anything_runs(encode):
    from flowdec_amd import _lib as L
    from flowdec_amd.ndac_pool import DecodePool, EncodePool
    m = ES.model("ndac75", "exact") if encode else DS.model("ndac75", "exact")
    pool = (EncodePool if encode else DecodePool)(m, capacity=2, block_frames=2, use_graph=False)
    pool._fin.fill_(-7)
    torch.cuda.synchronize()

    def row(**kw):
        rows = (L.FdNdacPoolRow * 1)()
        r = rows[0]
        r.ring, r.start, r.ring_cap, r.frames, r.nq, r.emit_lo, r.emit_count, r.out = pool._rings.data_ptr(), 0, pool.ring_cap, 3, 1, 0, 1, pool._fin.data_ptr()
        for k, v in kw.items():
            setattr(r, k, v)
        return rows

    for bad, word in ((dict(frames=0), "frames = 0"), (dict(frames=pool.T + 1), f"frames = {pool.T + 1}"), (dict(emit_lo=2, emit_count=2), "leave the window"),
                      (dict(nq=0), "nq = 0"), (dict(ring=None), "null")):
        with pool._on_side():
            with pytest.raises(RuntimeError, match=word):
                pool._call(row(**bad), 1, 1)
    torch.cuda.synchronize()
    assert pool.native_calls == 0 and pool.rows_run == 0 and bool((pool._fin == -7).all())


# ---- DecodePool in front of the enhance pool ----------------------------------------------------------------------------------------------
def test_codes_enhance_pool_equals_decode_stream_into_enhance_stream():
    from test_hip_longform import _flow
    from test_hip_stream import KW
    from flowdec_amd.ndac_pool import CodesEnhancePool
    from flowdec_amd.ndac_stream import DecodeStream
    from flowdec_amd.stream import EnhanceStream
    fm = _flow("bf16")
    dac = DS.model("ndac75", "mfma_decoder")
    streams = {7: DS.codes_of(dac, 4, 45, 9), 8: DS.codes_of(dac, 3, 41, 10)}
    want = {}
    for seed, codes in streams.items():
        dec, enh = DecodeStream(dac, n_quantizers=codes.shape[0], block_frames=3), EnhanceStream(fm, seed=seed, normfac="causal", **KW)
        parts = [enh.push(dec.push(codes[:, p:p + 4])) for p in range(0, codes.shape[1], 4)]
        parts += [enh.push(dec.flush()), enh.flush()]
        want[seed] = torch.cat(parts)
    pool = CodesEnhancePool(fm, dac, capacity=2, decode_block_frames=3, normfac="causal", **KW)
    sids = {seed: pool.open(seed=seed, n_quantizers=codes.shape[0]) for seed, codes in streams.items()}
    outs = {}
    for p in range(0, 45, 5):
        for seed, codes in streams.items():
            pool.push(sids[seed], codes[:, p:p + 5])
        drain(pool, outs)
    for seed, codes in streams.items():
        got = joined(outs, sids[seed], pool.flush(sids[seed]))
        assert got.shape == (codes.shape[1] * dac.hop_length,) and torch.equal(got, want[seed]), seed
    assert not torch.equal(want[7][:1000], want[8][:1000])
