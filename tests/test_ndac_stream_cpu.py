"""Streaming NDAC decode, host side: the decoder's halo rule (fd_ndac_decode_halo, computed by csrc/ndac_plan.h from the layer records;
called here through the library, which needs no GPU for it) against the oracle's actual receptive field and against recorded values, the
window planner (flowdec_amd/ndac_stream.py DecodePlanner) over random cuts, and the `stream_cli --codes` pieces that need no GPU (the byte-to-frame splitter, the parser's refusals)."""
import random

import numpy as np
import pytest

from oracle import ndac_oracle as N
from test_ndac_cpu import NDAC75_LIKE, SMALL, native_halo, scaled_sd


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from flowdec_amd import _lib
    return _lib.load()


def decode_halo(lib, decoder_rates):
    """fd_ndac_decode_halo (host only: the configuration alone, no weights, no GPU) -> (return code, (left, right))"""
    return native_halo(lib, dict(SMALL, decoder_rates=tuple(decoder_rates)), "decode")


# what the rule gave when it was written out by hand (commit e828d71: per block +-3 (9 + 3 + 1), floor((n + p) / s) - 1 .. floor((n + p) / s))
@pytest.mark.parametrize("rates,want", [((2,), (25, 25)), ((4, 2), (19, 19)), ((10, 8, 4, 2), (9, 9)), ((4, 2, 2), (21, 21))])
def test_native_decode_halo_values(lib, rates, want):
    assert decode_halo(lib, rates) == (0, want)


def test_native_decode_halo_refuses_an_odd_rate(lib):
    """(5, 4, 2): the decoded length is not frames * hop.  (The rule itself gives (15, 15) there: tests/test_model_host_cpu.py.)"""
    rc, _ = decode_halo(lib, (5, 4, 2))
    assert rc != 0 and b"decoder rate 5 is odd" in lib.fd_last_error()


@pytest.mark.parametrize("cfg,want", [(NDAC75_LIKE, (9, 9)), (dict(SMALL, decoder_rates=(4, 2, 2)), None)], ids=["ndac75_like", "small_422"])
def test_halo_rule_against_the_oracle(lib, cfg, want):
    rc, (hl, hr) = decode_halo(lib, cfg["decoder_rates"])
    assert rc == 0
    if want is not None:
        assert (hl, hr) == want
    T, f = 48, 24
    assert f - hr >= 1 and f + hl <= T - 2        # the affected range lies inside the signal, with an unaffected frame on each side
    o = N.DACOracle(scaled_sd(cfg, 3, 0.7), **cfg)
    up = int(np.prod(cfg["decoder_rates"]))
    rng = np.random.default_rng(0)
    z = rng.standard_normal((1, o.cfg["latent_dim"], T)).astype(np.float32)
    z2 = z.copy()
    z2[:, :, f] += 1.0
    ya, yb = o.decode(z)[0, 0], o.decode(z2)[0, 0]
    assert ya.shape == (T * up,)
    changed = np.nonzero(ya != yb)[0]
    assert changed.size
    first, last = changed[0] // up, changed[-1] // up
    # output frame g can see latent frame f iff g - hl <= f <= g + hr
    assert f - hr <= first and last <= f + hl, f"frames {first}..{last} changed, the rule allows {f - hr}..{f + hl}"
    assert first == f - hr and last == f + hl, f"frames {first}..{last} changed: the halo ({hl}, {hr}) is not tight to a frame"


def _cut(rng, total):
    """A random cut of `total` frames into pushes, empty pushes included."""
    cuts, left = [], total
    while left:
        n = rng.choice([0, 1, 1, 2, 3, 5, 8, 13, 40])
        n = min(n, left)
        cuts.append(n)
        left -= n
    if rng.random() < 0.5:
        cuts.insert(rng.randrange(len(cuts) + 1), 0)
    return cuts


def test_planner_over_random_cuts():
    from flowdec_amd.ndac_stream import DecodePlanner
    rng = random.Random(5)
    for trial in range(200):
        total, block = rng.randint(0, 80), rng.choice([1, 3, 8, 100])
        hl, hr = rng.choice([(9, 9), (15, 15), (0, 0), (2, 5)])
        p = DecodePlanner(hl, hr, block)
        assert p.latency_frames == block + hr - 1 and p.max_buffered == hl + block + hr - 1
        jobs, arrived_at_emit = [], []
        for n in _cut(rng, total):
            got = p.push(n)
            jobs += got
            arrived_at_emit += [p.received] * len(got)
            assert p.buffered <= p.max_buffered, (trial, p.buffered, p.max_buffered)
            assert p.received - p.emitted <= p.latency_frames           # latency: a frame still held has at most block + hr - 1 frames behind it
        got = p.flush()
        jobs += got
        arrived_at_emit += [total] * len(got)
        assert p.received == total and p.emitted == total
        # the emitted ranges tile [0, total) once, in order
        pos = 0
        for (w0, w1, e0, e1), arrived in zip(jobs, arrived_at_emit):
            assert e0 == pos and e1 > e0
            pos = e1
            # the window holds the full halo or touches a true edge, and lies within what had arrived
            assert w0 == max(0, e0 - hl) and w1 == min(arrived, e1 + hr) and w0 <= e0 and e1 <= w1 <= arrived
            assert e0 - w0 == hl or w0 == 0
            assert w1 - e1 == hr or w1 == total
        assert pos == total
        # the union of emits does not depend on the cut: the block grid plus one flush job
        one = DecodePlanner(hl, hr, block)
        ref = one.push(total) + one.flush()
        assert [(j[2], j[3]) for j in ref] == [(j[2], j[3]) for j in jobs]
        with pytest.raises(RuntimeError):
            p.push(1)
    with pytest.raises(ValueError):
        DecodePlanner(9, 9, 0)


def test_planner_block_jobs_sit_on_a_fixed_grid():
    """Before the flush every job emits exactly one block at a multiple of the block size, whatever the cut."""
    from flowdec_amd.ndac_stream import DecodePlanner
    rng = random.Random(1)
    for _ in range(50):
        total, block = rng.randint(30, 80), rng.choice([1, 3, 8])
        p = DecodePlanner(9, 9, block)
        jobs = [j for n in _cut(rng, total) for j in p.push(n)]
        assert all(e0 % block == 0 and e1 - e0 == block for _, _, e0, e1 in jobs)
        assert len(jobs) == (total - 9) // block
        tail = p.flush()
        assert len(tail) == 1 and tail[0][2] == len(jobs) * block and tail[0][3] == total


def test_cli_code_frame_splitter_carries_a_cut_frame():
    from flowdec_amd.stream_cli import CodeFrames

    def fail(msg):
        raise AssertionError(msg)

    nq = 3
    codes = np.random.default_rng(0).integers(0, 32, size=(11, nq)).astype("<i2")
    raw = codes.tobytes()
    for step in (1, 5, 6, 7, 64):                 # 5 and 7 bytes cut values and frames in two
        sp = CodeFrames(nq, 32, fail)
        got = [sp.feed(raw[i:i + step]) for i in range(0, len(raw), step)]
        assert all(g.shape[0] == nq and g.dtype == np.int64 for g in got)
        assert np.array_equal(np.concatenate(got, axis=1), codes.T.astype(np.int64)) and sp.rest == b"" and sp.frames == 11
    sp = CodeFrames(nq, 32, fail)
    assert sp.feed(raw[:-1]).shape == (nq, 10) and len(sp.rest) == 5


BASE = ["--ckpt", "c.ckpt", "--N", "2", "--seed", "1", "--normfac", "1.0", "--format", "f32le"]


def test_cli_parser_errors(capsys):
    from flowdec_amd import stream_cli
    assert stream_cli.parse_args(BASE).codes is False                            # without --codes: as before
    ok = stream_cli.parse_args(BASE + ["--codes", "--codec", "w.pth", "--n-quantizers", "4"])
    assert ok.codes and ok.codec == "w.pth" and ok.n_quantizers == 4 and ok.decode_block_frames == 8
    for argv, word in ((["--codes"], "--codec"), (["--codec", "w.pth"], "--codes")):
        with pytest.raises(SystemExit) as e:
            stream_cli.parse_args(BASE + argv)
        assert e.value.code == 2 and word in capsys.readouterr().err
    # a code outside [0, codebook_size) is the parser's error, with its frame index in the stream
    sp = stream_cli.CodeFrames(2, 1024, stream_cli.build_parser().error)
    assert sp.feed(np.array([[1, 2], [3, 1023]], dtype="<i2").tobytes()).shape == (2, 2)
    for bad in (1024, -1):
        sp = stream_cli.CodeFrames(2, 1024, stream_cli.build_parser().error)
        sp.feed(np.array([[1, 2], [3, 4], [5, 6]], dtype="<i2").tobytes())
        with pytest.raises(SystemExit) as e:
            sp.feed(np.array([[1, 2], [bad, 4]], dtype="<i2").tobytes())
        err = capsys.readouterr().err
        assert e.value.code == 2 and "frame 4" in err and str(bad) in err
