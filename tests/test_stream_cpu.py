"""Streaming planner and the host side of the streaming surface (flowdec_amd/longform.py StreamPlanner; flowdec_amd/stream.py;
flowdec_amd/stream_cli.py; no GPU).  The planner sees a running sample count and a final flush only, and must yield -- field for field --
the rows `plan_rows` cuts the finished recording into, with finished ranges that tile [0, n), whatever the cut of the input into pushes."""
import numpy as np
import pytest

from flowdec_amd.longform import StreamPlanner, plan_rows

HOP = 384
GEOMS = [(64, 8), (128, 32)]


def _lengths(rf, halo, rng):
    W, S = rf * HOP - 1, (rf - 2 * halo - 1) * HOP
    ns = {1, 2, HOP, W - 1, W, W + 1, W + 2, S + W - 1, S + W, S + W + 1, S + W + 2}
    for k in (1, 2, 3, 5):
        for d in (-HOP - 1, -HOP, -HOP + 1, -1, 0, 1, HOP - 1, HOP, HOP + 1):
            ns.add(k * S + W + d)
    ns.update(int(v) for v in rng.integers(1, 7 * S, 300))
    return sorted(ns)


def _cuts(n, rng, S):
    """Push schedules of n samples: one push; random sizes of three scales; 997-sample pushes."""
    yield [n]
    yield [997] * (n // 997) + ([n % 997] if n % 997 else [])
    for scale in (HOP, S, 3 * S):
        sizes, left = [], n
        while left:
            k = min(left, int(rng.integers(1, scale + 1)))
            sizes.append(k)
            left -= k
        yield sizes


def _drive(p, sizes, check=None):
    got = []
    for k in sizes:
        p.push(k)
        while True:
            r = p.next_row()
            if r is None:
                break
            got.append(r)
            if check:
                check(p, r)
    got.append(p.flush())
    if check:
        check(p, got[-1])
    return got


def _check_against_plan(got, n, rf, halo, xfade=2 * HOP):
    rows = plan_rows(n, HOP, rf, halo, xfade)
    half = xfade // 2
    assert len(got) == len(rows), (n, len(got), len(rows))
    for j, (g, r) in enumerate(zip(got, rows)):
        assert g.row == r, (n, j, g.row, r)
        assert (g.row.start, g.row.length, g.row.frame0, g.row.keep, g.row.xfade_lo, g.row.xfade_hi) == \
               (r.start, r.length, r.frame0, r.keep, r.xfade_lo, r.xfade_hi)
        assert g.index == j and g.last == (j == len(rows) - 1)
        lo = 0 if j == 0 else r.keep[0] - half
        hi = n if j == len(rows) - 1 else r.keep[1] - half
        assert g.finished == (lo, hi), (n, j, g.finished, (lo, hi))
        assert r.start <= lo and hi <= r.start + r.length          # what a row finishes lies inside it


@pytest.mark.parametrize("rf,halo", GEOMS)
def test_planner_equals_plan_rows_for_every_length_and_cut(rf, halo):
    rng = np.random.default_rng(rf)
    S = (rf - 2 * halo - 1) * HOP

    def retention(p, r):
        # every row that is yielded starts at or after what the session still keeps, and lies inside a ring of ring_samples from there
        assert retained[0] <= r.row.start, (retained, r)
        assert r.row.start + r.row.length - retained[0] <= p.ring_samples, (retained, r)
        retained[0] = p.retain_from
        assert retained[0] == max(r.index if not r.last else r.index - 1, 0) * S     # the start of the latest regular row

    for n in _lengths(rf, halo, rng):
        for sizes in _cuts(n, rng, S):
            assert sum(sizes) == n
            retained = [0]
            p = StreamPlanner(HOP, rf, halo)
            _check_against_plan(_drive(p, sizes, retention), n, rf, halo)
            assert p.n == n and p.done == n


def test_planner_one_sample_pushes_and_other_crossfades():
    rf, halo = 64, 8
    W, S = rf * HOP - 1, (rf - 2 * halo - 1) * HOP
    for n in (W, W + 1, S + W, S + W + 1, 2 * S + W - HOP):
        _check_against_plan(_drive(StreamPlanner(HOP, rf, halo), [1] * n), n, rf, halo)
    for xfade in (0, 2, 2 * halo * HOP):
        for n in (W + 1, 2 * S + W + 5):
            _check_against_plan(_drive(StreamPlanner(HOP, rf, halo, xfade), [n]), n, rf, halo, xfade)


def test_planner_readiness_delay_and_refusals():
    rf, halo = 64, 8
    p = StreamPlanner(HOP, rf, halo)
    W, S = p.W, p.S
    assert (W, S, p.Bo, p.half) == (rf * HOP - 1, (rf - 2 * halo - 1) * HOP, (rf - halo - 1) * HOP, HOP)
    p.push(W)
    assert not p.ready() and p.next_row() is None                 # W samples could still be the whole recording
    p.push(1)
    assert p.ready() and p.next_row().row.start == 0 and not p.ready()
    # the delay formula: the first sample row 0 leaves unfinished is final as soon as row 1 can run
    first_open = p.done
    assert first_open == p.Bo - p.half
    p.push(S - 1)
    assert not p.ready()
    p.push(1)
    assert p.ready() and p.n - first_open == p.delay_samples == (rf - halo) * HOP + p.half
    with pytest.raises(ValueError):
        p.flush()                                                 # a regular row is still ready
    p.next_row()
    p.flush()
    with pytest.raises(ValueError):
        p.push(1)
    with pytest.raises(ValueError):
        p.flush()
    with pytest.raises(ValueError):
        StreamPlanner(HOP, rf, halo).flush()                      # no input
    for bad in (dict(row_frames=65), dict(halo_frames=32), dict(xfade=3)):
        with pytest.raises(ValueError):
            StreamPlanner(HOP, **dict(dict(row_frames=64, halo_frames=8), **bad))
    # the noise contract: n / hop + T_pad stays below 2^31 absolute frames
    q = StreamPlanner(HOP, rf, halo)
    limit = (2 ** 31 - rf) * HOP
    q.push(limit - 1)
    with pytest.raises(RuntimeError, match="2\\^31"):
        q.push(1)
    assert q.n == limit - 1


def test_symbols_and_struct_layout():
    import ctypes as C
    from flowdec_amd import _lib
    lib = _lib.load()
    for name in ("fd_stream_gather", "fd_stream_emit"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert C.sizeof(_lib.FdStreamRow) == 64
    assert [getattr(_lib.FdStreamRow, f).offset for f, _ in _lib.FdStreamRow._fields_] == [0, 8, 16, 20, 24, 28, 32, 36, 40, 48, 56]
    # host-side refusals: nothing is launched
    assert lib.fd_stream_gather(None, 1, None, 10, None, None, None) == -1
    assert lib.fd_stream_emit(None, 1, None, 10, None, 0, None) == -1
    one = C.c_void_p(8)
    assert lib.fd_stream_gather(one, 1, one, 10, one, None, None) == -1      # peak without normfac_out
    assert lib.fd_stream_emit(one, 1, one, 10, None, 2, None) == -1          # a cross-fade without weights
    assert lib.fd_stream_emit(one, 1, one, 10, one, 3, None) == -1           # odd


def test_pool_refusals():
    import flowdec_amd
    from flowdec_amd.stream import EnhanceStream, StreamPool
    m = flowdec_amd.from_preset("flowdec_75m", nf=8)
    assert m.normalize_mode == "noisy"
    with pytest.raises(ValueError, match="fixed-step"):
        StreamPool(m, solver="dopri5", normfac="causal")
    with pytest.raises(ValueError, match="fixed-step"):
        EnhanceStream(m, seed=1, solver="tsit5", normfac=0.5)
    with pytest.raises(ValueError, match="normfac"):
        StreamPool(m, normfac=None)
    for bad in ("peak", 0.0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="normfac"):
            StreamPool(m, normfac=bad)
    with pytest.raises(ValueError, match="capacity"):
        StreamPool(m, capacity=0)
    m.normalize_mode = "none"
    with pytest.raises(ValueError, match="normfac"):
        StreamPool(m, normfac=0.5)


def test_stream_cli_arguments(capsys):
    from flowdec_amd import stream_cli
    base = ["--ckpt", "m.ckpt", "--N", "6", "--seed", "7", "--normfac", "causal", "--format", "s16le"]
    a = stream_cli.parse_args(base)
    assert (a.solver, a.row_frames, a.halo_frames, a.normfac, a.inp, a.out, a.block_samples) == ("euler", 256, 64, "causal", "-", "-", 4800)
    a = stream_cli.parse_args(["--ckpt", "c", "--N", "2", "--solver", "midpoint", "--seed", "1", "--row-frames", "64", "--halo-frames", "8", "--normfac",
                               "0.25", "--format", "f32le", "--in", "a.raw", "--out", "b.raw", "--block-samples", "100"])
    assert (a.solver, a.row_frames, a.halo_frames, a.normfac, a.format, a.inp, a.out, a.block_samples) == \
           ("midpoint", 64, 8, 0.25, "f32le", "a.raw", "b.raw", 100)

    def refused(argv, word):
        with pytest.raises(SystemExit) as e:
            stream_cli.parse_args(argv)
        assert e.value.code == 2 and word in capsys.readouterr().err

    refused([x for x in base if x not in ("--normfac", "causal")], "--normfac")
    refused(base[:-2], "--format")
    refused(base[:-4] + ["--normfac", "0", "--format", "s16le"], "--normfac")
    refused(base[:-4] + ["--normfac", "loud", "--format", "s16le"], "--normfac")
    refused(base + ["--solver", "dopri5"], "--solver")
    refused(base[:-1] + ["wav"], "--format")
    refused(base + ["--block-samples", "0"], "--block-samples")
    # s16le output: round to 16 bits, clipped
    import torch
    got = np.frombuffer(stream_cli.encode(torch.tensor([0.0, 0.5, -1.0, 1.0, 2.0, 1.5 / 32768]), "s16le"), dtype="<i2")
    assert got.tolist() == [0, 16384, -32768, 32767, 32767, 2]
    assert np.frombuffer(stream_cli.encode(torch.tensor([0.1, -3.0]), "f32le"), dtype="<f4").tolist() == [np.float32(0.1), -3.0]
