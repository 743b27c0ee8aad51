"""Streaming, long-form and ragged NDAC encode on the GPU (include/flowdec_hip.h fd_ndac_encode_ragged / fd_ndac_encode_halo;
flowdec_amd/ndac.py encode_ragged / encode_batch / encode_long; flowdec_amd/ndac_stream.py EncodeStream; flowdec_amd/codec_cli.py).

Every comparison is bit equality against the one-shot `DAC.encode`: a window of whole hops with the encoder's halo of real samples on
both sides reproduces the interior frames of the one-shot result because every kernel's per-output operation order is
position-independent (test 1, the premise), and a ragged row is its one-clip encode because every kernel bounds its input reads by the
clip's own length and the quantiser works per frame.  Builds: NDAC75_LIKE (vector path), WIDE_ENCODER (512 wide: matrix-core layers run
under precision="mfma"), WIDE_ENCODER_S5 (an odd stride)."""
import random

import numpy as np
import pytest
import torch

from test_hip_ndac import WIDE_ENCODER, WIDE_ENCODER_S5, build
from test_ndac_cpu import NDAC75_LIKE, SMALL, scaled_sd

pytestmark = pytest.mark.gpu

CFGS = {"ndac75": NDAC75_LIKE, "wide": WIDE_ENCODER, "s5": WIDE_ENCODER_S5, "beyond_chain": dict(SMALL, latent_dim=1056)}
HALOS = {"ndac75": (7, 7), "wide": (7, 7), "s5": (13, 13)}
BUILDS = [("ndac75", "exact"), ("wide", "exact"), ("wide", "mfma"), ("s5", "exact"), ("s5", "mfma")]
_models, _refs = {}, {}


def model(name, precision):
    if name not in _models:
        _models[name] = build(CFGS[name], 9, 0.7)[0]
    m = _models[name]
    m.precision = precision
    return m


def samples(n, seed):
    g = torch.Generator().manual_seed(seed)
    return 0.3 * torch.randn(n, generator=g)


def one_shot(name, precision, nq, total, seed=1):
    """(samples [total] on the host, dac.encode(dac.preprocess(samples), nq)[:3]) -- computed once, shared, never modified."""
    key = (name, precision, nq, total, seed)
    if key not in _refs:
        m = model(name, precision)
        x = samples(total, seed)
        _refs[key] = (x, tuple(t.clone() for t in m.encode(m.preprocess(x[None, None].cuda()), nq)[:3]))
    return _refs[key]


def bits(a, b):
    return a.shape == b.shape and (torch.equal(a.view(torch.int32), b.view(torch.int32)) if a.dtype == torch.float32 else torch.equal(a, b))


def shifted_windows_agree(m, w0, w1, total):
    """encode of the samples of frames [w0, w1) against encode of frames [0, total), on frames [w0 + HL, w1 - HR) -> frames compared."""
    hl, hr = m.encode_halo()
    hop = m.hop_length
    x = samples(total * hop, 3)[None, None].cuda()
    part, whole = m.encode(x[:, :, w0 * hop:w1 * hop].contiguous())[:3], m.encode(x)[:3]
    assert part[1].shape[-1] == w1 - w0 and whole[1].shape[-1] == total
    n = max(0, (w1 - hr) - (w0 + hl))
    for what, p, w in zip(("z", "codes", "latents"), part, whole):
        a, b = p[0, :, hl:hl + n], w[0, :, w0 + hl:w0 + hl + n]
        assert bits(a, b), f"{what}: {int((a != b).sum())} of {a.numel()} interior values depend on the window's position"
    assert not bits(part[2][0, :, 0], whole[2][0, :, w0])        # (the window's own first frame does differ: the comparison sees the halo)
    return n


@pytest.mark.parametrize("name,precision", BUILDS)
def test_shift_invariance(name, precision):
    """The premise: encode of the samples of frames [5, 31) equals encode of frames [0, 36) on frames [5 + HL, 31 - HR)."""
    m = model(name, precision)
    assert m.encode_halo() == HALOS[name]
    n = shifted_windows_agree(m, 5, 31, 36)
    assert n == (12 if name != "s5" else 0)
    if name == "s5":                     # halos of 13: the same comparison on a window that has an interior
        assert shifted_windows_agree(m, 5, 41, 47) == 10


def test_halo_is_the_mirror_and_a_rate_of_one_is_refused():
    from flowdec_amd.ndac import DAC
    for name in HALOS:
        m = model(name, "exact")
        assert m.encode_halo() == HALOS[name]
    bad = DAC(**dict(SMALL, encoder_rates=(2, 1, 4))).cuda()
    with pytest.raises(RuntimeError, match="rate of 1"):
        bad.encode_halo()


@pytest.mark.parametrize("name,precision", BUILDS + [("beyond_chain", "exact")])
def test_ragged_rows_are_their_one_clip_encodes(name, precision):
    """(beyond_chain: latent_dim 1056, past rvq_chain_kernel's width -- the ragged entry falls back to step launches under the table.)"""
    from flowdec_amd import _lib as L
    m = model(name, precision)
    assert L.load().fd_rvq_chain_supported(m.latent_dim, m.codebook_dim) == (name != "beyond_chain")
    hop, T, frames = m.hop_length, 23, (23, 9, 1)
    x = samples(3 * T * hop, 7).reshape(3, 1, T * hop).cuda()
    alone = [m.encode(x[b:b + 1, :, :f * hop].contiguous())[:3] for b, f in enumerate(frames)]
    xr = x.clone()
    for b, f in enumerate(frames):
        xr[b, :, f * hop:] = float("nan")          # what lies behind a clip is never read as data
    got = m.encode_ragged(xr, frames)
    assert got[0].shape == (3, m.latent_dim, T) and got[1].shape == (3, m.n_codebooks, T) and got[1].dtype == torch.int64
    for b, f in enumerate(frames):
        for what, g, a in zip(("z", "codes", "latents"), got, alone[b]):
            assert bits(g[b:b + 1, :, :f], a), f"{what} of row {b} ({f} frames): {int((g[b:b + 1, :, :f] != a).sum())} values differ from the one-clip encode"
            assert torch.count_nonzero(g[b, :, f:]) == 0, f"{what} of row {b} is not 0 behind frame {f}"
    assert torch.isfinite(got[0]).all() and torch.isfinite(got[2]).all()
    dense = m.encode(x)[:3]
    assert all(bits(g, d) for g, d in zip(m.encode_ragged(x, (T, T, T)), dense))              # all-full frames: the dense encode
    by_dev = m.encode_ragged(xr, torch.tensor(frames, dtype=torch.int32, device="cuda"), ws=m.encode_workspace(4, (T + 3) * hop))      # a device table, a larger workspace
    assert all(bits(g, d) for g, d in zip(by_dev, got))
    g3 = m.encode_ragged(xr, frames, n_quantizers=3)
    assert bits(g3[1], got[1][:, :3]) and bits(g3[2], got[2][:, :3 * m.codebook_dim])


@pytest.mark.parametrize("bad", [(23, 0, 5), (23, 24, 5), (-1, 3, 5)])
def test_ragged_refuses_bad_frame_counts_with_outputs_untouched(bad):
    from flowdec_amd import _lib as L
    m = model("ndac75", "exact")
    lib, h = L.load(), m.handle()
    hop, T = m.hop_length, 23
    x = samples(3 * T * hop, 7).reshape(3, T * hop).cuda()
    z = torch.full((3, m.latent_dim, T), 7.0, device="cuda")
    codes = torch.full((3, m.n_codebooks, T), -7, dtype=torch.int32, device="cuda")
    lat = torch.full((3, m.n_codebooks * m.codebook_dim, T), 7.0, device="cuda")
    ws = m.encode_workspace(3, T * hop)
    fr = torch.tensor(bad, dtype=torch.int32, device="cuda")
    rc = lib.fd_ndac_encode_ragged(h, L.ptr(x), L.ptr(fr), 3, T * hop, 0, L.ptr(z), L.ptr(codes), L.ptr(lat), L.ptr(ws), ws.numel(), L.stream())
    torch.cuda.synchronize()
    assert rc != 0 and b"frames[" in lib.fd_last_error()
    assert bool((z == 7.0).all()) and bool((codes == -7).all()) and bool((lat == 7.0).all())
    with pytest.raises(RuntimeError, match="outside"):
        m.encode_ragged(x[:, None], bad)
    with pytest.raises(RuntimeError, match="hop"):
        m.encode_ragged(x[:, None, :-1], (1, 1, 1))


def test_encode_batch_returns_the_callers_order():
    m = model("ndac75", "exact")
    hop = m.hop_length
    lens = (9 * hop, 23 * hop - 17, 1, 14 * hop + 1, 9 * hop)
    waves = [samples(n, 20 + i)[None].cuda() for i, n in enumerate(lens)]
    for nq in (None, 3):
        outs = m.encode_batch(waves, n_quantizers=nq, batch=2)
        assert len(outs) == len(waves)
        for w, c in zip(waves, outs):
            want = m.encode(m.preprocess(w[None]), nq)[1][0]
            assert c.dtype == torch.int64 and c.shape == want.shape == (m.n_codebooks if nq is None else nq, -(-w.shape[1] // hop)) and torch.equal(c, want)
    with pytest.raises(RuntimeError):
        m.encode_batch([waves[0][:, :0]])


def cut(rng, total):
    sizes, left = [], total
    while left:
        n = min(rng.choice([0, 1, 2, 3, 7, 639, 640, 641, 5000]), left)
        sizes.append(n)
        left -= n
    return sizes + [0]


@pytest.mark.parametrize("block", [1, 8])
@pytest.mark.parametrize("nq", [3, None])
@pytest.mark.parametrize("name,precision", BUILDS)
def test_stream_equals_one_shot_encode(name, precision, nq, block):
    from flowdec_amd.ndac_stream import EncodeStream
    m = model(name, precision)
    hop = m.hop_length
    total = 40 * hop - hop // 3                                 # about 40 frames; the last one partial
    x, (_, want, _) = one_shot(name, precision, nq, total)
    want = want[0]
    rng = random.Random(block * 10 + (nq or 0))
    for label, sizes in (("one push", [total]), ("random", cut(rng, total)), ("random", cut(rng, total))):
        st = EncodeStream(m, n_quantizers=nq, block_frames=block, rows_per_call=4)
        assert st.delay_samples == (block + HALOS[name][1] - 1) * hop
        outs, pos = [], 0
        for i, n in enumerate(sizes):
            c = x[pos:pos + n]
            pos += n
            outs.append(st.push(c.cuda() if i % 2 else c))           # device and host pushes mixed
            assert outs[-1].is_cuda and outs[-1].dtype == torch.int64 and outs[-1].shape[0] == want.shape[0]
            assert st.buffered_samples <= (st.planner.max_buffered + 1) * hop, (label, st.buffered_samples)
        outs.append(st.flush())
        got = torch.cat(outs, dim=1)
        assert got.shape == want.shape == (want.shape[0], 40) and torch.equal(got, want), f"{label}: {int((got != want).sum())} of {want.numel()} codes differ"
        assert st.frames_encoded >= 40 and st.windows_run >= 1
        if label == "random" and block + HALOS[name][1] < 40:
            assert sum(o.shape[1] > 0 for o in outs[:-1]) >= 1              # codes did leave before the flush
        with pytest.raises(RuntimeError):
            st.push(x[:1])


@pytest.mark.parametrize("block", [1, 8])
def test_stream_short_totals(block):
    from flowdec_amd.ndac_stream import EncodeStream
    m = model("ndac75", "exact")
    hop, right = m.hop_length, HALOS["ndac75"][1]
    for total in (0, 1, hop - 1, hop, hop + 1, (block + right) * hop - 1, (block + right) * hop + 1):
        st = EncodeStream(m, n_quantizers=3, block_frames=block)
        if total == 0:
            assert st.push(torch.zeros(0)).shape == (3, 0)
            y = st.flush()
            assert y.shape == (3, 0) and y.is_cuda and y.dtype == torch.int64
            continue
        x, (_, want, _) = one_shot("ndac75", "exact", 3, total, seed=total)
        a, b = st.push(x[:total // 2]), st.push(x[total // 2:])
        if total < (block + right) * hop:
            assert a.shape[1] == 0 and b.shape[1] == 0           # fewer complete frames than block + halo: nothing is final yet
        else:
            assert b.shape[1] == block                           # the first block left with the sample that completed frame block + right
        got = torch.cat([a, b, st.flush()], dim=1)
        assert torch.equal(got, want[0]), total


@pytest.mark.parametrize("name,precision", [("ndac75", "exact"), ("wide", "mfma")])
def test_encode_long_equals_one_shot(name, precision, monkeypatch):
    from flowdec_amd import _lib as L
    m = model(name, precision)
    hop = m.hop_length
    x, want = one_shot(name, precision, 3, 60 * hop)
    xd = x[None, None].cuda()
    lib = L.load()
    real, asked = lib.fd_ndac_workspace_bytes, []

    def spy(h, B, Ls):
        asked.append((B, Ls))
        return real(h, B, Ls)

    monkeypatch.setattr(lib, "fd_ndac_workspace_bytes", spy)
    got = m.encode_long(xd, 3, window_frames=24, rows_per_call=2)
    assert asked == [(2, 24 * hop)]                              # one workspace, sized for (rows_per_call, window_frames) ...
    assert got[3] is None and got[4] is None and all(bits(g, w) for g, w in zip(got[:3], want))
    asked.clear()
    g50 = m.encode_long(xd[:, :, :50 * hop].contiguous(), 3, window_frames=24, rows_per_call=2)
    assert asked == [(2, 24 * hop)]                              # ... whatever the length
    monkeypatch.undo()
    assert all(bits(g, w) for g, w in zip(g50[:3], m.encode(xd[:, :, :50 * hop].contiguous(), 3)[:3]))
    with pytest.raises(ValueError, match="halos"):
        m.encode_long(xd, 3, window_frames=14)
    # a recording that fits one window is one plain encode call
    monkeypatch.setattr(m, "encode_ragged", lambda *a, **k: pytest.fail("encode_long ran a ragged call for a recording that fits one window"))
    for wf in (60, 1024):
        assert all(bits(g, w) for g, w in zip(m.encode_long(xd, 3, window_frames=wf)[:3], want))


@pytest.mark.parametrize("fmt", ["f32le", "s16le"])
def test_codec_cli_round_trip(tmp_path, fmt):
    """`codec_cli`'s bytes are the one-shot codes, and fed to DecodeStream they give decode(from_codes(codes)) bit for bit."""
    from flowdec_amd import codec_cli
    from flowdec_amd.ndac import DAC
    from flowdec_amd.ndac_stream import DecodeStream
    from flowdec_amd.stream_cli import CodeFrames
    cfg, nq = NDAC75_LIKE, 4
    sd = scaled_sd(cfg, 5, 0.6)
    torch.save({"state_dict": {k: torch.from_numpy(v) for k, v in sd.items()},
                "metadata": {"kwargs": dict(cfg, encoder_rates=list(cfg["encoder_rates"]), decoder_rates=list(cfg["decoder_rates"]))}}, tmp_path / "weights.pth")
    dac = DAC.load(str(tmp_path / "weights.pth")).cuda()
    hop = dac.hop_length
    total = 30 * hop + 123
    x = samples(total, 9)
    if fmt == "s16le":
        pcm = np.clip(np.rint(x.numpy().astype(np.float64) * 32768.0), -32768, 32767).astype("<i2")
        x = torch.from_numpy(pcm.astype(np.float32) / np.float32(32768.0))
    else:
        pcm = x.numpy().astype("<f4")
    pcm.tofile(tmp_path / "in.raw")
    # 4801 samples per read: no read ends on a frame
    n = codec_cli.run(["--codec", str(tmp_path / "weights.pth"), "--format", fmt, "--n-quantizers", str(nq), "--encode-block-frames", "3",
                       "--in", str(tmp_path / "in.raw"), "--out", str(tmp_path / "codes.raw"), "--block-samples", "4801"])
    raw = (tmp_path / "codes.raw").read_bytes()
    want = dac.encode(dac.preprocess(x[None, None].cuda()), nq)[1][0]
    assert n == 31 and want.shape == (nq, 31) and raw == want.cpu().numpy().T.astype("<i2").tobytes()
    codes = torch.from_numpy(CodeFrames(nq, dac.codebook_size, pytest.fail).feed(raw))            # stream_cli --codes reads them back
    st = DecodeStream(dac, n_quantizers=nq, block_frames=3)
    y = torch.cat([st.push(codes[:, :11]), st.push(codes[:, 11:]), st.flush()])
    assert torch.equal(y, dac.decode(dac.quantizer.from_codes(want[None])[0])[0, 0])
