"""Streaming, long-form and ragged NDAC decode on the GPU (include/flowdec_hip.h fd_ndac_decode_ragged / fd_ndac_decode_halo;
flowdec_amd/ndac.py decode_ragged / decode_batch / decode_long; flowdec_amd/ndac_stream.py; `stream_cli --codes`).

Every comparison is bit equality against the one-shot `DAC.decode`: a window with the decoder's halo of real context on both sides
reproduces the interior of the one-shot result because every kernel's per-output operation order is position-independent (test 1,
the premise), and a ragged row is its one-clip decode because every kernel bounds its input reads by the clip's own length.
Builds: NDAC75_LIKE (vector path), WIDE_DECODER (768 wide: matrix-core layers run), SMALL (odd rates, ragged call only)."""
import random

import numpy as np
import pytest
import torch

from test_hip_ndac import WIDE_DECODER, build
from test_ndac_cpu import NDAC75_LIKE, SMALL

pytestmark = pytest.mark.gpu

CFGS = {"ndac75": NDAC75_LIKE, "wide": WIDE_DECODER, "small": SMALL}
_models, _refs = {}, {}


def model(name, precision):
    if name not in _models:
        _models[name] = build(CFGS[name], 5, 0.6)[0]
    m = _models[name]
    m.precision = precision
    return m


def latents(m, B, T, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, m.latent_dim, T, generator=g).cuda()


def codes_of(m, nq, T, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, m.codebook_size, (nq, T), generator=g)


def one_shot(name, precision, nq, T, seed=1):
    """(codes [nq, T] on the host, dac.decode(dac.quantizer.from_codes(codes)[0])[0, 0]) -- computed once, shared, never modified."""
    key = (name, precision, nq, T, seed)
    if key not in _refs:
        m = model(name, precision)
        c = codes_of(m, nq, T, seed)
        _refs[key] = (c, m.decode(m.quantizer.from_codes(c[None].cuda())[0])[0, 0].clone())
    return _refs[key]


def cut(rng, total):
    sizes, left = [], total
    while left:
        n = min(rng.choice([0, 1, 2, 3, 7, 11, 20]), left)
        sizes.append(n)
        left -= n
    return sizes + [0]


@pytest.mark.parametrize("precision", ["exact", "mfma_decoder"])
@pytest.mark.parametrize("name", ["ndac75", "wide"])
def test_shift_invariance(name, precision):
    """The premise: decode of frames [5, 31) equals decode of frames [0, 36) on the samples of frames [5 + HL, 31 - HR)."""
    m = model(name, precision)
    hl, hr = m.decode_halo()
    assert (hl, hr) == (9, 9)
    hop = m.hop_length
    z = latents(m, 1, 36, 3)
    part, whole = m.decode(z[:, :, 5:31])[0, 0], m.decode(z[:, :, 0:36])[0, 0]
    assert part.numel() == 26 * hop and whole.numel() == 36 * hop
    a, b = part[hl * hop:(26 - hr) * hop], whole[(5 + hl) * hop:(31 - hr) * hop]
    assert a.numel() == 8 * hop and torch.equal(a, b), f"{int((a != b).sum())} of {a.numel()} interior samples depend on the window's position"
    assert not torch.equal(part[:hop], whole[5 * hop:6 * hop])        # (the window's own edge does differ: the comparison sees the halo)


def test_halo_refuses_odd_rates():
    m = model("small", "exact")
    with pytest.raises(RuntimeError, match="rate 5 is odd"):
        m.decode_halo()
    from flowdec_amd.ndac_stream import DecodeStream
    with pytest.raises(RuntimeError, match="odd"):
        DecodeStream(m)


@pytest.mark.parametrize("precision", ["exact", "mfma_decoder"])
@pytest.mark.parametrize("name", ["ndac75", "wide", "small"])
def test_ragged_rows_are_their_one_clip_decodes(name, precision):
    from flowdec_amd import _lib as L
    m = model(name, precision)
    lib, h = L.load(), m.handle()
    T, frames = 23, (23, 9, 1)
    z = latents(m, 3, T, 7)
    alone = [m.decode(z[b:b + 1, :, :f].contiguous())[0] for b, f in enumerate(frames)]
    zr = z.clone()
    for b, f in enumerate(frames):
        zr[b, :, f:] = float("nan")            # what lies behind a clip is never read as data
    y = m.decode_ragged(zr, frames)
    Lo = lib.fd_ndac_decoded_length(h, T)
    assert y.shape == (3, 1, Lo)
    for b, f in enumerate(frames):
        n = lib.fd_ndac_decoded_length(h, f)
        assert alone[b].shape == (1, n) and (n == f * m.hop_length) == (name != "small")      # SMALL: the odd-rate length rule
        assert torch.equal(y[b, :, :n], alone[b]), f"row {b} ({f} frames): {int((y[b, :, :n] != alone[b]).sum())} samples differ from the one-clip decode"
        assert torch.count_nonzero(y[b, :, n:]) == 0 and torch.isfinite(y[b]).all()
    assert torch.equal(m.decode_ragged(z, (T, T, T)), m.decode(z))
    assert torch.equal(m.decode_ragged(z, torch.tensor(frames, dtype=torch.int32, device="cuda")), y)      # a device table


def test_decode_batch_returns_the_callers_order():
    m = model("ndac75", "mfma_decoder")
    lens = (9, 23, 1, 14, 9)
    zs = [latents(m, 1, t, 20 + i)[0] for i, t in enumerate(lens)]
    outs = m.decode_batch(zs, batch=2)
    assert len(outs) == len(zs)
    for z, y in zip(zs, outs):
        assert y.shape == (1, z.shape[1] * m.hop_length) and torch.equal(y, m.decode(z[None])[0])
    with pytest.raises(RuntimeError):
        m.decode_batch([zs[0][:, :0]])


@pytest.mark.parametrize("bad", [(23, 0, 5), (23, 24, 5), (-1, 3, 5)])
def test_ragged_refuses_bad_frame_counts_with_outputs_untouched(bad):
    from flowdec_amd import _lib as L
    m = model("ndac75", "mfma_decoder")
    lib, h = L.load(), m.handle()
    T = 23
    z = latents(m, 3, T, 7)
    out = torch.full((3, 1, lib.fd_ndac_decoded_length(h, T)), 7.0, device="cuda")
    ws = m.decode_workspace(3, T)
    fr = torch.tensor(bad, dtype=torch.int32, device="cuda")
    rc = lib.fd_ndac_decode_ragged(h, L.ptr(z), L.ptr(fr), 3, T, L.ptr(out), L.ptr(ws), ws.numel(), L.stream())
    torch.cuda.synchronize()
    assert rc != 0 and b"frames[" in lib.fd_last_error() and bool((out == 7.0).all())
    with pytest.raises(RuntimeError, match="outside"):
        m.decode_ragged(z, bad)


@pytest.mark.parametrize("block", [1, 4, 64])
@pytest.mark.parametrize("nq", [4, None])
@pytest.mark.parametrize("name,precision", [("ndac75", "exact"), ("ndac75", "mfma_decoder"), ("wide", "exact"), ("wide", "mfma_decoder")])
def test_stream_equals_one_shot_decode(name, precision, nq, block):
    from flowdec_amd.ndac_stream import DecodeStream
    m = model(name, precision)
    nq_rows = m.n_codebooks if nq is None else nq
    T = 40
    codes, want = one_shot(name, precision, nq_rows, T)
    rng = random.Random(block * 10 + nq_rows)
    for label, sizes in (("one push", [T]), ("frame by frame", [1] * T), ("random", cut(rng, T)), ("random", cut(rng, T))):
        st = DecodeStream(m, n_quantizers=nq, block_frames=block, rows_per_call=4)
        assert st.delay_samples == (block + 9 - 1) * m.hop_length
        outs, pos = [], 0
        for i, n in enumerate(sizes):
            c = codes[:, pos:pos + n]
            pos += n
            outs.append(st.push(c.cuda() if i % 2 else c[None]))          # device [nq, n] and host [1, nq, n] pushes mixed
            assert outs[-1].is_cuda and outs[-1].dtype == torch.float32 and outs[-1].ndim == 1
            assert st.buffered_frames <= st.planner.max_buffered, (label, st.buffered_frames)
        outs.append(st.flush())
        got = torch.cat(outs)
        assert got.shape == want.shape and torch.equal(got, want), f"{label}: {int((got != want).sum())} of {want.numel()} samples differ"
        if label == "frame by frame" and block < T:
            assert sum(o.numel() > 0 for o in outs[:-1]) > 1            # samples did leave before the flush
            assert outs[block + 9 - 1].numel() == block * m.hop_length and not any(o.numel() for o in outs[:block + 9 - 1])
        with pytest.raises(RuntimeError):
            st.push(codes[:, :1])


@pytest.mark.parametrize("T", [0, 1, 3])
def test_stream_short_totals(T):
    from flowdec_amd.ndac_stream import DecodeStream
    m = model("ndac75", "mfma_decoder")
    st = DecodeStream(m, block_frames=4)
    if T == 0:
        assert st.push(torch.zeros(m.n_codebooks, 0, dtype=torch.int64)).numel() == 0
        y = st.flush()
        assert y.numel() == 0 and y.is_cuda and y.dtype == torch.float32
        return
    codes, want = one_shot("ndac75", "mfma_decoder", m.n_codebooks, T, seed=T)
    assert st.push(codes).numel() == 0              # fewer frames than the halo: nothing is final yet
    assert torch.equal(st.flush(), want)


def test_stream_host_and_device_pushes_agree_and_codes_are_checked():
    from flowdec_amd.ndac_stream import DecodeStream
    m = model("ndac75", "mfma_decoder")
    codes, want = one_shot("ndac75", "mfma_decoder", 4, 40)
    got = []
    for c in (codes, codes.cuda(), codes.to(torch.int16), codes.to(torch.int32).cuda()[None]):
        st = DecodeStream(m, block_frames=8)
        got.append(torch.cat([st.push(c[..., :25]), st.push(c[..., 25:]), st.flush()]))
    assert all(torch.equal(g, want) for g in got)
    st = DecodeStream(m)                                # the first push fixes the number of code rows
    st.push(codes[:, :3])
    with pytest.raises(RuntimeError):
        st.push(codes[:3, :3])
    with pytest.raises(RuntimeError, match="codebooks"):
        DecodeStream(m).push(torch.zeros(m.n_codebooks + 1, 2, dtype=torch.int64))
    with pytest.raises(RuntimeError, match="codebooks"):
        DecodeStream(m, n_quantizers=m.n_codebooks + 1)
    with pytest.raises(TypeError):
        DecodeStream(m).push(torch.zeros(4, 2))


@pytest.mark.parametrize("name,precision", [("ndac75", "exact"), ("wide", "mfma_decoder")])
def test_decode_long_equals_one_shot(name, precision, monkeypatch):
    from flowdec_amd import _lib as L
    m = model(name, precision)
    codes, want = one_shot(name, precision, 4, 70)
    lib = L.load()
    real, asked = lib.fd_ndac_workspace_bytes, []

    def spy(h, B, Ls):
        asked.append((B, Ls))
        return real(h, B, Ls)

    monkeypatch.setattr(lib, "fd_ndac_workspace_bytes", spy)
    y = m.decode_long(codes, window_frames=24, rows_per_call=3)
    assert y.shape == (1, 1, 70 * m.hop_length) and torch.equal(y[0, 0], want)
    assert asked == [(3, 24 * m.hop_length)]                      # one workspace, sized for (rows_per_call, window_frames) ...
    asked.clear()
    y50 = m.decode_long(codes[:, :50].cuda()[None], window_frames=24, rows_per_call=3)
    assert asked == [(3, 24 * m.hop_length)]                      # ... whatever the length
    assert torch.equal(y50[0, 0], m.decode(m.quantizer.from_codes(codes[None, :, :50].cuda())[0])[0, 0])
    with pytest.raises(ValueError, match="halos"):
        m.decode_long(codes, window_frames=18)
    # a recording that fits one window is one plain decode call
    monkeypatch.setattr(m, "decode_ragged", lambda *a, **k: pytest.fail("decode_long ran a ragged call for a recording that fits one window"))
    for wf in (70, 1024):
        assert torch.equal(m.decode_long(codes, window_frames=wf)[0, 0], want)


def test_stream_cli_codes_equal_the_pcm_path(tmp_path):
    """`stream_cli --codes --codec W` on a code file = `stream_cli` on the one-shot decoded PCM as f32le, byte for byte."""
    import flowdec_amd
    from flowdec_amd import stream_cli
    from oracle import flowdec_oracle as O
    from test_ndac_cpu import scaled_sd
    fm = flowdec_amd.from_preset("flowdec_75m", precision="bf16", nf=8)
    fm.load_state_dict({k: torch.from_numpy(v) for k, v in O.random_state_dict(seed=8, nf=8).items()}, strict=False)
    fm = fm.cuda()
    cfg, nq, T = NDAC75_LIKE, 4, 45
    sd = scaled_sd(cfg, 5, 0.6)
    torch.save({"state_dict": {k: torch.from_numpy(v) for k, v in sd.items()},
                "metadata": {"kwargs": dict(cfg, encoder_rates=list(cfg["encoder_rates"]), decoder_rates=list(cfg["decoder_rates"]))}}, tmp_path / "weights.pth")
    from flowdec_amd.ndac import DAC
    dac = DAC.load(str(tmp_path / "weights.pth")).cuda()
    assert dac.sample_rate == fm.sampling_rate
    codes = codes_of(dac, nq, T, 9)
    codes.numpy().T.astype("<i2").tofile(tmp_path / "codes.raw")                    # frame-major, nq values per frame
    pcm = dac.decode(dac.quantizer.from_codes(codes[None].cuda())[0])[0, 0]
    pcm.cpu().numpy().astype("<f4").tofile(tmp_path / "pcm.raw")
    common = ["--ckpt", "unused", "--N", "2", "--solver", "euler", "--seed", "7", "--row-frames", "64", "--halo-frames", "16", "--normfac", "causal",
              "--format", "f32le"]
    n_pcm = stream_cli.run(common + ["--in", str(tmp_path / "pcm.raw"), "--out", str(tmp_path / "a.raw"), "--block-samples", "4801"], model=fm)
    # 37 int16 values per read: every read but a few cuts a 4-value frame in two
    n_codes = stream_cli.run(common + ["--codes", "--codec", str(tmp_path / "weights.pth"), "--n-quantizers", str(nq), "--decode-block-frames", "3",
                                       "--in", str(tmp_path / "codes.raw"), "--out", str(tmp_path / "b.raw"), "--block-samples", "37"], model=fm)
    a, b = (tmp_path / "a.raw").read_bytes(), (tmp_path / "b.raw").read_bytes()
    assert n_pcm == n_codes == T * dac.hop_length and len(a) == 4 * n_pcm
    assert a == b
    out = np.frombuffer(a, dtype="<f4")
    assert np.isfinite(out).all() and np.abs(out).max() > 0
    bad = codes.numpy().T.astype("<i2").copy()
    bad[17, 2] = cfg["codebook_size"]
    bad.tofile(tmp_path / "bad.raw")
    with pytest.raises(SystemExit):
        stream_cli.run(common + ["--codes", "--codec", str(tmp_path / "weights.pth"), "--n-quantizers", str(nq), "--in", str(tmp_path / "bad.raw"),
                                 "--out", str(tmp_path / "c.raw")], model=fm)
