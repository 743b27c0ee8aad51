"""Streaming NDAC encode, host side: the encoder's halo rule (fd_ndac_encode_halo, computed by csrc/ndac_plan.h from the layer records;
called through the library, which needs no GPU for it) against recorded values and the oracle's actual receptive field, `EncodeStream`'s
bookkeeping (flowdec_amd/ndac_stream.py) over random cuts in samples on a stand-in codec whose encode IS the oracle, the host-only rules of the C ABI (fd_ndac_encode_halo, fd_rvq_chain_supported) and the `codec_cli`
pieces that need no GPU (the parser's refusals, the sample reader, the frame-major int16 writer)."""
import math
import random

import numpy as np
import pytest
import torch

from oracle import ndac_oracle as N
from test_ndac_cpu import NDAC75_LIKE, SMALL, native_halo, scaled_sd


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from flowdec_amd import _lib
    return _lib.load()


def _native_halo(lib, rates):
    """fd_ndac_encode_halo (host only: the configuration alone, no weights, no GPU) -> (return code, (left, right))"""
    return native_halo(lib, dict(SMALL, encoder_rates=tuple(rates)), "encode")


@pytest.mark.parametrize("rates,want", [((2, 4, 8, 10), (7, 7)), ((2, 4, 8, 8), (8, 8)), ((2, 4, 5), (13, 13))])
def test_encode_halo_mirror(lib, rates, want):
    """The three halos DESIGN.md quotes (they were once asserted of a Python restatement of the rule; now of the rule itself)."""
    assert _native_halo(lib, rates) == (0, want)


# what the rule gave when it was written out by hand (commit e828d71: [t - 1, t + 1] walked back through strided conv, +-3 (9 + 3 + 1), +-3)
HALO_AT_E828D71 = {(2, 4, 8, 10): (7, 7), (2, 4, 8, 8): (8, 8), (2, 4, 5): (13, 13), (3,): (16, 16), (16, 2): (23, 23), (5, 3, 7): (10, 10)}


@pytest.mark.parametrize("rates", [(2, 4, 8, 10), (2, 4, 8, 8), (2, 4, 5), (3,), (16, 2), (5, 3, 7)])
def test_native_halo_equals_the_mirror(lib, rates):
    """The rule derived from the layer records gives what the hand-written rule (and its Python mirror) gave, odd and single rates included."""
    assert _native_halo(lib, rates) == (0, HALO_AT_E828D71[rates])


def test_native_halo_refuses_a_rate_of_one(lib):
    rc, _ = _native_halo(lib, (2, 1, 4))
    assert rc != 0 and b"rate of 1" in lib.fd_last_error()


def test_rvq_chain_supported_rule(lib):
    """The [D][8] float32 residual tile beside the step's small arrays within 64 KiB of LDS, and D / 32 <= 32 accumulators a thread."""
    for D, cd, want in ((64, 8, 1), (128, 8, 1), (512, 8, 1), (1024, 8, 1), (1000, 3, 1), (1, 1, 1), (1025, 8, 0), (2048, 8, 0), (1024, 9, 0), (1024, 0, 0),
                        (0, 8, 0)):
        assert lib.fd_rvq_chain_supported(D, cd) == want, (D, cd)


@pytest.mark.parametrize("cfg,want", [(NDAC75_LIKE, (7, 7)), (SMALL, (13, 13))], ids=["ndac75_like", "small"])
def test_encode_halo_rule_against_the_oracle(lib, cfg, want):
    rc, (hl, hr) = _native_halo(lib, cfg["encoder_rates"])
    assert rc == 0 and (hl, hr) == want
    T, f = 40, 20
    assert f - hr >= 1 and f + hl <= T - 2        # the affected range lies inside the signal, with an unaffected frame on each side
    o = N.DACOracle(scaled_sd(cfg, 3, 0.7), **cfg)
    hop = o.hop_length
    rng = np.random.default_rng(0)
    x = (0.3 * rng.standard_normal((1, 1, T * hop))).astype(np.float32)
    x2 = x.copy()
    x2[:, :, f * hop:(f + 1) * hop] += 0.5        # every sample of frame f
    za, zb = o.encoder(x)[0], o.encoder(x2)[0]
    assert za.shape == (o.cfg["latent_dim"], T)
    changed = np.nonzero((za != zb).any(axis=0))[0]
    assert changed.size
    first, last = int(changed[0]), int(changed[-1])
    # latent frame g can see the samples of frame f iff g - hl <= f <= g + hr
    assert f - hr <= first and last <= f + hl, f"frames {first}..{last} changed, the rule allows {f - hr}..{f + hl}"
    assert first == f - hr and last == f + hl, f"frames {first}..{last} changed: the halo ({hl}, {hr}) is not tight to a frame"
    # a window with the halos reproduces the interior latents; cut at the interior frame's own edge it does not
    w0, w1 = f - hl, f + 2 + hr
    zw = o.encoder(x[:, :, w0 * hop:w1 * hop])[0]
    assert np.array_equal(zw[:, hl:hl + 2], za[:, f:f + 2]), "a window with the full halo does not reproduce its interior latents"
    assert not np.array_equal(zw[:, 0], za[:, w0]) and not np.array_equal(zw[:, -1], za[:, w1 - 1])      # (its own edge frames do differ)
    zc = o.encoder(x[:, :, f * hop:(f + 2) * hop])[0]
    assert zc.shape[1] == 2 and not np.array_equal(zc[:, 0], za[:, f]) and not np.array_equal(zc[:, 1], za[:, f + 1])
    zl = o.encoder(x[:, :, (w0 + 1) * hop:w1 * hop])[0]      # one frame short on the left: the first interior frame feels the edge
    assert not np.array_equal(zl[:, hl - 1], za[:, f])


class OracleCodec:
    """Stands in for `flowdec_amd.ndac.DAC` under EncodeStream: `encode` / `encode_ragged` are the oracle, row by row, on the host."""

    def __init__(self, lib, cfg, seed=3, gain=0.7):
        self.lib = lib
        self.o = N.DACOracle(scaled_sd(cfg, seed, gain), **cfg)
        self.hop_length, self.n_codebooks, self.sample_rate = self.o.hop_length, cfg["n_codebooks"], cfg["sample_rate"]
        self.encoder_rates = cfg["encoder_rates"]
        self.device = torch.device("cpu")
        self.calls = []

    def encode_halo(self):
        rc, halo = _native_halo(self.lib, self.encoder_rates)      # the code that ships, not a restatement of it
        assert rc == 0
        return halo

    def encode(self, audio, n_quantizers=None):
        z, codes, lat, _, _ = self.o.encode(audio.numpy(), n_quantizers)
        return torch.from_numpy(z), torch.from_numpy(codes), torch.from_numpy(lat), None, None

    def encode_ragged(self, audio, frames, n_quantizers=None, ws=None):
        B, _, Lw = audio.shape
        self.calls.append(list(frames))
        outs = None
        for b, f in enumerate(frames):
            assert 1 <= f <= Lw // self.hop_length
            r = self.encode(audio[b:b + 1, :, :f * self.hop_length], n_quantizers)[:3]
            if outs is None:
                outs = [torch.zeros((B,) + tuple(t.shape[1:-1]) + (Lw // self.hop_length,), dtype=t.dtype) for t in r]
            for o_, t in zip(outs, r):
                o_[b, ..., :f] = t[0]
        return tuple(outs)


def _cut_samples(rng, total):
    cuts, left = [], total
    while left:
        n = min(rng.choice([0, 1, 2, 3, 7, 39, 40, 41, 97, 333, 1000]), left)
        cuts.append(n)
        left -= n
    return cuts + [0]


@pytest.mark.parametrize("block", [1, 8])
def test_encode_stream_bookkeeping_over_random_cuts(lib, block):
    from flowdec_amd.ndac_stream import EncodeStream
    dac = OracleCodec(lib, SMALL)
    hop = dac.hop_length
    assert hop == 40 and dac.encode_halo() == (13, 13)
    rng = random.Random(block)
    nprng = np.random.default_rng(block)
    for total, nq in ((61 * hop + 17, 3), (50 * hop, None), (hop - 1, 2), (0, None)):
        x = (0.3 * nprng.standard_normal(total)).astype(np.float32)
        nq_rows = dac.n_codebooks if nq is None else nq
        want = dac.o.encode(dac.o.preprocess(x[None, None]), nq)[1][0] if total else np.zeros((nq_rows, 0), np.int64)
        st = EncodeStream(dac, n_quantizers=nq, block_frames=block, rows_per_call=3)
        assert st.delay_samples == (block + 13 - 1) * hop
        outs, pos = [], 0
        for n in _cut_samples(rng, total):
            outs.append(st.push(torch.from_numpy(x[pos:pos + n])))
            pos += n
            assert outs[-1].dtype == torch.int64 and outs[-1].shape[0] == nq_rows
            assert st.buffered_samples <= (st.planner.max_buffered + 1) * hop, (st.buffered_samples, st.planner.max_buffered)
            assert st.samples_received == pos and st.planner.received == pos // hop
        outs.append(st.flush())
        got = torch.cat(outs, dim=1).numpy()
        assert got.shape == want.shape and np.array_equal(got, want), f"total {total}: {int((got != want).sum())} of {want.size} codes differ"
        assert st.buffered_samples == 0 and st.planner.emitted == math.ceil(total / hop)
        if total > (block + 13) * hop:
            assert sum(o.shape[1] > 0 for o in outs[:-1]) >= 1          # codes did leave before the flush
            assert st.frames_encoded >= math.ceil(total / hop) and st.windows_run >= 1
        with pytest.raises(RuntimeError):
            st.push(torch.zeros(3))
        with pytest.raises(RuntimeError):
            st.flush()
    assert any(len(c) > 1 for c in dac.calls)                          # several blocks finished by one push shared a ragged call
    with pytest.raises(TypeError):
        EncodeStream(dac).push(torch.zeros(4, dtype=torch.float64))
    with pytest.raises(TypeError):
        EncodeStream(dac).push(torch.zeros(2, 2))
    with pytest.raises(RuntimeError, match="codebooks"):
        EncodeStream(dac, n_quantizers=dac.n_codebooks + 1)
    with pytest.raises(ValueError):
        EncodeStream(dac, rows_per_call=0)


def test_encode_long_windows_on_the_oracle(lib):
    """encode_long's jobs tile the recording: z, codes and latents equal the one-shot encode; one workspace request, sized for the window."""
    from flowdec_amd.ndac_stream import encode_long
    dac = OracleCodec(lib, SMALL)
    asked = []
    dac.encode_workspace = lambda B, Ls: asked.append((B, Ls))
    hop = dac.hop_length
    x = torch.from_numpy((0.3 * np.random.default_rng(2).standard_normal((1, 1, 90 * hop))).astype(np.float32))
    want = dac.encode(x, 3)
    got = encode_long(dac, x, 3, window_frames=40, rows_per_call=2)
    assert asked == [(2, 40 * hop)] and got[3] is None and got[4] is None
    assert all(len(c) <= 2 and max(c) <= 40 for c in dac.calls) and len(dac.calls) >= 2
    assert torch.equal(got[1], want[1]) and torch.equal(got[0], want[0]) and torch.equal(got[2], want[2])
    dac.calls.clear()
    assert torch.equal(encode_long(dac, x, 3, window_frames=90)[1], want[1]) and not dac.calls      # fits one window: the plain encode
    with pytest.raises(ValueError, match="halos"):
        encode_long(dac, x, 3, window_frames=26)
    with pytest.raises(RuntimeError, match="hop"):
        encode_long(dac, x[:, :, :-1], 3)


# ---- codec_cli ---------------------------------------------------------------------------------------------------------------------------
BASE = ["--codec", "w.pth", "--format", "s16le"]


def test_codec_cli_parser_errors(capsys):
    from flowdec_amd import codec_cli
    ok = codec_cli.parse_args(BASE)
    assert ok.codec == "w.pth" and ok.n_quantizers is None and ok.encode_block_frames == 8 and ok.block_samples == 4800 and ok.inp == "-" and ok.out == "-"
    ok = codec_cli.parse_args(BASE + ["--n-quantizers", "4", "--encode-block-frames", "1", "--in", "a.raw", "--out", "b.raw", "--block-samples", "7"])
    assert (ok.n_quantizers, ok.encode_block_frames, ok.inp, ok.out, ok.block_samples) == (4, 1, "a.raw", "b.raw", 7)
    for argv, word in ((["--format", "s16le"], "--codec"), (["--codec", "w.pth"], "--format"), (BASE + ["--n-quantizers", "0"], "--n-quantizers"),
                       (BASE + ["--encode-block-frames", "0"], "--encode-block-frames"), (BASE + ["--block-samples", "0"], "--block-samples"),
                       (["--codec", "w.pth", "--format", "s24le"], "--format"), (BASE + ["--decode"], "--decode"), (BASE + ["--in-rate", "44100"], "--in-rate")):
        with pytest.raises(SystemExit) as e:
            codec_cli.parse_args(argv)
        assert e.value.code == 2 and word in capsys.readouterr().err


def test_codec_cli_writer_is_the_stream_cli_reader_format():
    """code_bytes: int16, little endian, frame-major, Q values per frame -- what stream_cli's CodeFrames splits back into [Q, n]."""
    from flowdec_amd import codec_cli
    from flowdec_amd.stream_cli import CodeFrames
    codes = torch.from_numpy(np.random.default_rng(0).integers(0, 1024, size=(3, 11)))
    raw = codec_cli.code_bytes(codes)
    assert len(raw) == 2 * 3 * 11 and raw[:6] == np.array([int(codes[0, 0]), int(codes[1, 0]), int(codes[2, 0])], dtype="<i2").tobytes()
    sp = CodeFrames(3, 1024, pytest.fail)
    assert np.array_equal(sp.feed(raw), codes.numpy()) and sp.rest == b""
    assert codec_cli.code_bytes(torch.zeros(3, 0, dtype=torch.int64)) == b""
    assert codec_cli.code_bytes(torch.tensor([[32767]])) == b"\xff\x7f"
    for bad in (32768, -1):
        with pytest.raises(ValueError, match="int16"):
            codec_cli.code_bytes(torch.tensor([[1, bad]]))


def test_codec_cli_sample_reader():
    from flowdec_amd import codec_cli
    s16 = np.array([0, 1, -1, 32767, -32768, 12345], dtype="<i2")
    x = codec_cli.decode_pcm(s16.tobytes(), "s16le")
    assert x.dtype == torch.float32 and np.array_equal(x.numpy(), s16.astype(np.float32) / np.float32(32768))
    f32 = np.array([0.0, 0.25, -1.0, 1e-8], dtype="<f4")
    y = codec_cli.decode_pcm(f32.tobytes(), "f32le")
    assert y.dtype == torch.float32 and np.array_equal(y.numpy(), f32)


def test_codec_cli_refuses_a_codebook_beyond_int16(tmp_path, capsys):
    from types import SimpleNamespace
    from flowdec_amd import codec_cli
    big = SimpleNamespace(codebook_size=32769, n_codebooks=4)
    with pytest.raises(SystemExit) as e:
        codec_cli.run(BASE + ["--in", str(tmp_path / "none.raw")], dac=big)
    assert e.value.code == 2 and "int16" in capsys.readouterr().err
    ok = SimpleNamespace(codebook_size=1024, n_codebooks=4)
    with pytest.raises(SystemExit) as e:
        codec_cli.run(BASE + ["--n-quantizers", "5", "--in", str(tmp_path / "none.raw")], dac=ok)
    assert e.value.code == 2 and "4 codebooks" in capsys.readouterr().err
