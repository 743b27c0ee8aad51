"""Sub-sample alignment with polarity on the host (flowdec_amd.align: frac_bank, refine_lag, frac_shift, support_frac, align_triple_frac,
align_pair_frac) and the command-line switches on the HOST_SCORER.  No GPU.

Synthetic pairs: white noise band-limited in the frequency domain and delayed by an FFT phase ramp (an exact band-limited delay of the
periodic signal; 128 samples are cut from both ends so that the wrap-around is not seen).  A delay with a fractional part of 0.5 is given
the band 0.9 Nyquist and the full band goes to a delay of 1 / Q: a 64-tap Hann-windowed sinc has a transition band of about 2 / W = 6 %
of Nyquist in which a half-sample shift is attenuated, while a shift of 1 / 64 sample is nearly the impulse at every frequency.  The
-7.72 delay has the search M = 40 > 7.72 + W, so that every tap of the refinement lies inside the correlation (a peak within W of the
edge of the search is interpolated from fewer taps and can land on a neighbouring grid step)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from test_align_cpu import FD_EINVAL, FD_ENOMEM, SR, make_delayed_triples
from test_eval_cpu import read_csv, write_wav

Q, W = 64, 32
# (L, M, delay, band in Nyquist, inverted)
PAIRS = [(600, 8, 3.3, 0.9, False), (4096, 40, -7.72, 0.45, True), (2048, 16, 0.5, 0.9, False), (1000, 12, 2.015625, 1.0, True), (1000, 8, -0.3, 0.7, False)]


def delayed_pair(L, d, band, seed, invert=False):
    """-> (x, y) float32 [L]: y[n] = +-x(n - d), x white noise below `band` Nyquist, peak 1."""
    rng = np.random.default_rng(seed)
    n = L + 256
    X = np.fft.rfft(rng.standard_normal(n))
    X[np.arange(len(X)) > band * (len(X) - 1)] = 0.0
    x = np.fft.irfft(X, n)
    y = np.fft.irfft(X * np.exp(-2j * np.pi * np.fft.rfftfreq(n) * d), n)
    g = 1.0 / np.abs(x).max()
    return (g * x[128:128 + L]).astype(np.float32), ((-g if invert else g) * y[128:128 + L]).astype(np.float32)


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def test_bank_properties():
    from flowdec_amd import align
    H = align.frac_bank()
    assert H.shape == (Q, 2 * W) and H.dtype == np.float64 and align.frac_bank(Q, W) is H and not H.flags.writeable
    want = np.zeros(2 * W)
    want[W - 1] = 1.0
    assert np.array_equal(H[0], want)
    assert np.abs(H.sum(axis=1) - 1.0).max() <= 1e-5
    for j in range(1, Q):
        for k in range(-W + 2, W):                                  # 1 - k stays inside [-W + 1, W]
            assert abs(H[j][k + W - 1] - H[Q - j][(1 - k) + W - 1]) <= 1e-15, (j, k)
    u = 5 - 17 / Q
    assert H[17][5 + W - 1] == np.sinc(u) * (0.5 * (1.0 + np.cos(np.pi * u / W)))
    small = align.frac_bank(2, 1)                                   # |u| >= W is exactly 0: tap k = 0 of row 1 has u = -0.5, tap 1 has u = 0.5
    assert small.shape == (2, 2) and small[0].tolist() == [1.0, 0.0] and small[1][0] == small[1][1] > 0.3
    for bad in ((1, 32), (1025, 32), (64, 0), (64, 257)):
        with pytest.raises(ValueError):
            align.frac_bank(*bad)


def test_refine_lag_on_hand_made_correlations():
    from flowdec_amd import align
    M = 40
    flat = np.full(2 * M + 1, 3.0)
    assert align.refine_lag(np.zeros(2 * M + 1), Q, W) == (0, 1) and align.refine_lag(np.zeros(2 * M + 1), Q, W, polarity=True) == (0, 1)
    assert align.refine_lag(np.full(2 * M + 1, np.nan), Q, W, polarity=True) == (0, 1)
    l0, sign = align.refine_lag(flat, Q, W)                         # all equal: l0 = 0 by pick_lag; the row sums differ from 1 by < 1e-5 only
    assert sign == 1 and abs(l0) < Q
    # a single peak: every interpolated value is below the peak itself (|H| < 1 off the impulse row), so q = 0
    c = np.zeros(2 * M + 1)
    c[M + 7] = 2.0
    assert align.refine_lag(c, Q, W) == (7 * Q, 1) and align.refine_lag(-c, Q, W, polarity=True) == (7 * Q, -1)
    # polarity=False ignores a negative peak: the largest c is one of the zeros, the nearest to 0 with +l first is l = 0
    lag_q, sign = align.refine_lag(-c, Q, W)
    assert sign == 1 and lag_q // Q in (-1, 0) and lag_q != 7 * Q
    # two equal neighbours: the maximum lies half way, and the tie of the integer pick went to the smaller |l|
    c = np.zeros(2 * M + 1)
    c[M + 3] = c[M + 4] = 1.0
    assert align.pick_lag(c) == 3 and align.refine_lag(c, Q, W) == (3 * Q + Q // 2, 1)
    c = np.zeros(2 * M + 1)
    c[M - 3] = c[M - 4] = -1.0
    assert align.refine_lag(c, Q, W, polarity=True) == (-3 * Q - Q // 2, -1)
    # ties among the candidates, on the smallest grid (Q = 2, W = 1: row 1 is two equal taps h = 0.318 at k = 0, 1, so r(1) = h (c[l0] +
    # c[l0 + 1]) and r(-1) = h (c[l0 - 1] + c[l0]) are the same two-term sums for equal neighbours): +q before -q, else the larger r
    c = np.full(2 * M + 1, -10.0)
    c[M + 3], c[M + 2], c[M + 4] = -1.0, -1.5, -1.5
    assert align.refine_lag(c, 2, 1) == (3 * 2 + 1, 1)
    c[M + 2] = -1.4
    assert align.refine_lag(c, 2, 1) == (3 * 2 - 1, 1)
    c[M + 2] = c[M + 4] = -3.0                                      # h (-4) < -1: the integer peak itself
    assert align.refine_lag(c, 2, 1) == (3 * 2, 1)
    # a NaN r counts as -inf: a NaN beside the peak is a tap of every candidate (the impulse row multiplies it by 0.0, NaN again), so all
    # are -inf and q = 0
    c = np.zeros(2 * M + 1)
    c[M + 5], c[M + 6] = 4.0, np.nan
    assert align.refine_lag(c, Q, W) == (5 * Q, 1)
    # l0 = +-M: no candidate beyond the search
    for edge in (M, -M):
        c = np.zeros(2 * M + 1)
        c[M + edge] = 1.0
        c[M + edge - np.sign(edge)] = 0.99
        lag_q, _ = align.refine_lag(c, Q, W)
        assert abs(lag_q) <= M * Q and abs(lag_q) > (M - 1) * Q and lag_q != edge * Q
        c[M + edge - np.sign(edge)] = 0.0
        assert align.refine_lag(c, Q, W) == (edge * Q, 1)
    with pytest.raises(ValueError):
        align.refine_lag(np.zeros(4), Q, W)


def test_frac_shift_definition_and_support():
    from flowdec_amd import align
    rng = np.random.default_rng(5)
    s = rng.standard_normal(200).astype(np.float32)
    H = align.frac_bank(Q, W)
    # the definition, one sample at a time in Python floats
    for lag_q, sign, n0, n1 in ((3 * Q + 17, 1, 0, 200), (-5 * Q - 1, -1, -40, 30), (Q - 1, 1, 150, 260), (2 * Q, -1, -3, 203)):
        base, j = divmod(lag_q, Q)
        want = []
        for n in range(n0, n1):
            acc = 0.0
            for t in range(2 * W):
                m = n + base + t - W + 1
                acc = acc + (float(s[m]) if 0 <= m < len(s) else 0.0) * float(H[j][t])
            want.append(np.float32(sign * acc))
        got = align.frac_shift(s, lag_q, sign, Q, W, n0, n1)
        assert got.dtype == np.float32 and np.array_equal(got, np.array(want, np.float32)), lag_q
    assert np.array_equal(align.frac_shift(s, 2 * Q, 1, Q, W, 0, 198), s[2:])          # j = 0: the impulse row copies
    assert not align.frac_shift(s, 7, 1, Q, W, 500, 600).any() and align.frac_shift(s, 7, 1, Q, W, 9, 3).shape == (0,)
    # support: no tap reads outside the signal exactly on [lo, hi)
    for lag_q in (3 * Q + 17, -5 * Q - 1, 2 * Q, -2 * Q, 1, Q - 1):
        lo, hi = align.support_frac(200, lag_q, Q, W)
        base, j = divmod(lag_q, Q)
        reach = (0, 0) if j == 0 else (-W + 1, W)
        assert lo + base + reach[0] == 0 and hi - 1 + base + reach[1] == 199
    assert align.common_support_frac(1000, (1000, 990), (3 * Q, -2 * Q + 1), Q, W) == (max(0, -3, W - 1 + 2), min(1000, 997, 990 - W + 2))


@pytest.fixture(scope="module")
def synthetic():
    """The five pairs with their correlation, computed once."""
    from flowdec_amd import align
    out = []
    for i, (L, M, d, band, inv) in enumerate(PAIRS):
        x, y = delayed_pair(L, d, band, 40 + i, inv)
        out.append((x, y, align.xcorr(x, y, M)))
    return out


@pytest.mark.parametrize("k", range(len(PAIRS)))
def test_synthetic_pairs_delay_sign_and_residual(synthetic, k):
    from flowdec_amd import align
    L, M, d, band, inv = PAIRS[k]
    x, y, c = synthetic[k]
    lag_q, sign = align.refine_lag(c, Q, W, polarity=True)
    xa, ya = align.align_pair_frac(x, y, lag_q, sign, Q, W)
    inner = slice(2 * W, -2 * W)
    res = rel(ya[inner], xa[inner])
    l0, s0 = align.pick_polarity(c)
    xi, yi = align.align_pair_frac(x, y, l0 * Q, s0, Q, W)
    res_int = rel(yi[inner], xi[inner])
    print(f"L {L} M {M} d {d} band {band}: lag {lag_q / Q} (error {abs(lag_q / Q - d) * Q:.3f} / Q) sign {sign}; residual {res:.3g}, integer {res_int:.3g}")
    assert abs(lag_q / Q - d) <= 1.0 / Q and sign == (-1 if inv else 1) == s0
    assert len(xa) == len(ya) > L - 2 * W - 2 * abs(d) - 2 and res <= 2e-2
    if 0.3 <= d % 1.0 <= 0.7:
        assert res_int >= 0.2
    # without polarity an inverted pair is not found (its peak is negative)
    if inv:
        assert align.refine_lag(c, Q, W)[1] == 1 and abs(align.refine_lag(c, Q, W)[0] / Q - d) > 0.5
    # host_lags_frac is refine_lag of xcorr
    got_q, got_s, cs = align.host_lags_frac([x], [torch.from_numpy(y)], M, Q, W, True, return_xcorr=True)
    assert got_q.dtype == np.int64 and got_s.dtype == np.int32 and got_q.tolist() == [lag_q] and got_s.tolist() == [sign] and np.array_equal(cs[0], c)


def test_integer_delays_give_the_very_arrays_of_align_triple():
    from flowdec_amd import align
    rng = np.random.default_rng(9)
    h, x, y = (torch.from_numpy(rng.standard_normal(n).astype(np.float32)) for n in (1000, 990, 1010))

    def boom(*a, **k):
        raise AssertionError("a whole-sample delay with sign +1 must be cut as a view")

    for lag_h, lag_y in ((5, -3), (0, 0), (-12, 20), (2000, 0)):
        want = align.align_triple(h, x, y, lag_h, lag_y)
        got = align.align_triple_frac(h, x, y, lag_h * Q, lag_y * Q, 1, 1, Q, W, shift=boom)
        for a, b in zip(got, want):
            assert a.shape == b.shape and torch.equal(a, b) and (a.numel() == 0 or a.data_ptr() == b.data_ptr())
        gn = align.align_triple_frac(h.numpy(), x.numpy(), y.numpy(), lag_h * Q, lag_y * Q, 1, 1, Q, W, shift=boom)
        assert all(isinstance(a, np.ndarray) and np.array_equal(a, b.numpy()) for a, b in zip(gn, want))
    # an inverted signal at a whole delay is the negated view; a fractional one is shorter by the taps' reach and goes through `shift`
    gh, gx, gy = align.align_triple_frac(h, x, y, 5 * Q, -3 * Q, -1, 1, Q, W)
    wh, wx, wy = align.align_triple(h, x, y, 5, -3)
    assert torch.equal(gh, -wh) and torch.equal(gx, wx) and torch.equal(gy, wy) and gy.data_ptr() == wy.data_ptr()
    gh, gx, gy = align.align_triple_frac(h, x, y, 5 * Q + 1, -3 * Q, 1, 1, Q, W)
    n0, n1 = align.common_support_frac(990, (1000, 1010), (5 * Q + 1, -3 * Q), Q, W)
    assert (n0, n1) == (W - 1 - 5, 1000 - W - 5) and gh.shape == gx.shape == gy.shape == (n1 - n0,) and gh.dtype == torch.float32
    assert np.array_equal(gh.numpy(), align.frac_shift(h, 5 * Q + 1, 1, Q, W, n0, n1)) and torch.equal(gy, y[n0 - 3:n1 - 3])
    xa, ya = align.align_pair_frac(x, y, -3 * Q, 1, Q, W, shift=boom)
    assert torch.equal(xa, x[3:990]) and torch.equal(ya, y[0:987])


def test_symbols_in_the_header_the_table_and_the_build():
    import __graft_entry__ as g
    g.build()
    from flowdec_amd import _lib
    lib = _lib.load()
    src = open(os.path.join(g.ROOT, "include", "flowdec_hip.h")).read()
    for name in ("fd_xcorr_frac_workspace_bytes", "fd_xcorr_lags_frac", "fd_frac_shift"):
        assert name + "(" in src and hasattr(lib, name) and name in _lib.SIGNATURES
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
    assert "fracshift.hip" in __import__("flowdec_amd.build", fromlist=["SOURCES"]).SOURCES
    # refusals need no GPU: every call below refuses before a launch
    err = lambda: lib.fd_last_error().decode()
    p = C.c_void_p(16)
    need = lib.fd_xcorr_frac_workspace_bytes(2, 1000, 900, 300)
    assert need == lib.fd_xcorr_workspace_bytes(2, 1000, 900, 300) > 0 and lib.fd_xcorr_frac_workspace_bytes(2, 1000, 900, 0) == 0
    call = lambda bank=p, Q=64, W=32, n=1 << 40, lag_q=p, sign=p: lib.fd_xcorr_lags_frac(p, p, p, p, 2, 1000, 900, 300, bank, Q, W, 1, None, lag_q, sign, p, n, None)
    assert call(bank=None) == FD_EINVAL and "fd_xcorr_lags_frac" in err() and "bank" in err()
    for kw, word in ((dict(Q=1), "Q 1"), (dict(Q=1025), "Q 1025"), (dict(W=0), "W 0"), (dict(W=257), "W 257")):
        assert call(**kw) == FD_EINVAL and "fd_xcorr_lags_frac" in err() and word in err(), (kw, err())
    assert call(lag_q=None) == FD_EINVAL and call(sign=None) == FD_EINVAL and "null pointer" in err()
    assert call(n=need - 1) == FD_ENOMEM and "workspace" in err()
    shift = lambda s=p, W=32, Ls=100, Lo=100, B=2: lib.fd_frac_shift(s, p, B, Ls, p, p, W, p, p, p, p, Lo, None)
    for kw, word in ((dict(s=None), "null pointer"), (dict(W=0), "W 0"), (dict(W=257), "W 257"), (dict(Ls=0), "Ls 0"), (dict(Lo=0), "Lo 0"), (dict(B=0), "B 0")):
        assert shift(**kw) == FD_EINVAL and "fd_frac_shift" in err() and word in err(), (kw, err())


def frac_triples(tmp_path):
    """Two triples at 48 kHz: x_hat late by 2.5 samples and inverted, y early by 3 whole samples; then both at whole delays (4, -2)."""
    lines = []
    for i, (dh, dy, inv) in enumerate(((2.5, -3.0, True), (4.0, -2.0, False))):
        x, h = delayed_pair(6000, dh, 0.8, 70 + i, inv)
        _, y = delayed_pair(6000, dy, 0.8, 70 + i)
        y = y + (0.01 * np.random.default_rng(90 + i).standard_normal(6000)).astype(np.float32)
        h = h + (0.001 * np.random.default_rng(95 + i).standard_normal(6000)).astype(np.float32)
        paths = [tmp_path / f"clean_{i}.wav", tmp_path / f"noisy_{i}.wav", tmp_path / f"enh_{i}.wav"]
        for path, s in zip(paths, (0.5 * x, 0.5 * y, 0.5 * h)):
            write_wav(path, s, SR)
        lines.append(" ---> ".join(str(q) for q in paths))
    lst = tmp_path / "frac_triples.txt"
    lst.write_text("\n".join(lines) + "\n")
    return lst


def test_eval_cli_new_columns_on_the_host_scorer(tmp_path, capsys):
    from flowdec_amd import eval_cli
    lst = frac_triples(tmp_path)
    out = {k: tmp_path / f"{k}.csv" for k in ("align", "frac", "pol", "both")}
    flags = dict(align=["--align", "1"], frac=["--align", "1", "--align-frac"], pol=["--align", "1", "--align-polarity"],
                 both=["--estoi", "--align", "1", "--align-frac", "--align-polarity"])
    res, caps, heads, rows = {}, {}, {}, {}
    for k in out:
        res[k] = eval_cli.run(["--triples", str(lst), "--out", str(out[k])] + flags[k], scorer=eval_cli.HOST_SCORER)
        caps[k] = capsys.readouterr()
        heads[k], rows[k] = read_csv(out[k])
    base = eval_cli.CSV_HEADER
    assert tuple(heads["align"]) == tuple(heads["frac"]) == base + ("lag_x_hat", "lag_y")
    assert tuple(heads["pol"]) == base + ("lag_x_hat", "lag_y", "pol_x_hat", "pol_y") == base + eval_cli.LAG_NAMES + eval_cli.POL_NAMES
    assert tuple(heads["both"]) == base + ("estoi", "lag_x_hat", "lag_y", "pol_x_hat", "pol_y")
    # the lags: lag_q / Q printed in full, whole lags as integers; the polarity columns 1 or -1
    assert [r[-4:] for r in rows["both"]] == [["2.5", "-3", "-1", "1"], ["4", "-2", "1", "1"]]
    assert [r[-2:] for r in rows["frac"]][1] == ["4", "-2"] and [r[-4:] for r in rows["pol"]][1] == ["4", "-2", "1", "1"]
    assert rows["pol"][0][-4:] in (["2", "-3", "-1", "1"], ["3", "-3", "-1", "1"])
    # whole-sample delays: the same bits under --align-frac as under --align
    assert rows["frac"][1] == rows["align"][1] and rows["pol"][1][:-2] == rows["align"][1]
    # the half-sample, inverted x_hat: SI-SDR only with both switches
    assert float(rows["both"][0][4]) > 30.0 > 10.0 > float(rows["pol"][0][4]) and float(rows["frac"][0][4]) < 30.0
    assert res["both"].lags == [("lag_x_hat", "2.5", "4", 2), ("lag_y", "-3", "-2", 2)] and res["both"].inverted == [("pol_x_hat", 1), ("pol_y", 0)]
    assert "pol_x_hat    inverted in 1 of 2 rows" in caps["both"].out and "inverted" not in caps["frac"].out and res["frac"].inverted == []
    assert "min = 2.5  max = 4  non-zero in 2 of 2" in caps["both"].out
    for bad in (["--align-frac"], ["--align-polarity"], ["--align", "1", "--align-frac", "--align-q", "1"], ["--align", "1", "--align-frac", "--align-taps", "0"]):
        with pytest.raises(SystemExit):
            eval_cli.run(["--triples", str(lst), "--out", str(tmp_path / "x.csv")] + bad, scorer=eval_cli.HOST_SCORER)
    assert "need --align MS" in capsys.readouterr().err


def test_align_alone_keeps_its_bytes_and_does_not_reach_the_new_paths(tmp_path, capsys):
    from flowdec_amd import eval_cli
    lst = make_delayed_triples(tmp_path)

    def boom(*a, **k):
        raise AssertionError("a new code path was reached by --align alone")

    H = eval_cli.HOST_SCORER
    old = eval_cli.Scorer(H.si_sxr, H.logspec, H.estoi, H.spectral, H.align)                    # the fields of before: the new ones are None
    trap = eval_cli.Scorer(H.si_sxr, H.logspec, H.estoi, H.spectral, H.align, boom, boom)
    assert old.align_frac is None and old.shift is None and H.align_frac is not None and eval_cli.GPU_SCORER.shift is not None
    for flags in (["--align", "2"], ["--estoi", "--spectral", "--align", "2"], []):
        outs = []
        for name, scorer in (("a.csv", H), ("b.csv", old), ("c.csv", trap)):
            eval_cli.run(["--triples", str(lst), "--out", str(tmp_path / name)] + flags, scorer=scorer)
            outs.append(capsys.readouterr().out.replace(name, "x.csv"))
        assert (tmp_path / "a.csv").read_bytes() == (tmp_path / "b.csv").read_bytes() == (tmp_path / "c.csv").read_bytes()
        assert outs[0] == outs[1] == outs[2] and "pol_" not in outs[0]
    with pytest.raises(AssertionError):
        eval_cli.run(["--triples", str(lst), "--out", str(tmp_path / "d.csv"), "--align", "2", "--align-frac"], scorer=trap)
    with pytest.raises(ValueError):
        eval_cli.run(["--triples", str(lst), "--out", str(tmp_path / "d.csv"), "--align", "2", "--align-polarity"], scorer=old)


def test_enhance_cli_passes_the_switches_on(monkeypatch):
    from flowdec_amd import enhance_cli, eval_cli
    seen = []
    monkeypatch.setattr(eval_cli, "run", lambda argv, **k: seen.append(list(argv)))
    import argparse
    ns = argparse.Namespace(outdir="o", batch_files=4, device=0, eval_estoi=False, eval_spectral=False, eval_align=1.0, eval_align_frac=True,
                            eval_align_polarity=True)
    monkeypatch.setattr(torch.cuda, "device", lambda d: __import__("contextlib").nullcontext())
    enhance_cli.evaluate_triples(ns, "")
    assert seen and seen[0][-4:] == ["--align", "1.0", "--align-frac", "--align-polarity"]
    ns.eval_align_frac = ns.eval_align_polarity = False
    enhance_cli.evaluate_triples(ns, "")
    assert seen[1][-2:] == ["--align", "1.0"]
    flags = {a.dest for a in enhance_cli.build_parser()._actions}
    assert {"eval_align_frac", "eval_align_polarity"} <= flags


def test_pair_aligner_on_the_host_functions_and_the_parsers(capsys):
    import argparse
    from flowdec_amd import align, estimate_cli, loss_cli
    for mod, req in ((estimate_cli, ["--pairs-file", "p", "--alpha", "0.3", "--nfft", "1534", "--hop", "384"]), (loss_cli, ["--ckpt", "c", "--pairs-file", "p"])):
        a = mod.build_parser().parse_args(req)
        assert a.align is None and not a.align_frac and not a.align_polarity and (a.align_q, a.align_taps) == (64, 32)
        a = mod.build_parser().parse_args(req + ["--align", "1.5", "--align-frac", "--align-polarity", "--align-q", "32", "--align-taps", "16"])
        assert (a.align, a.align_frac, a.align_polarity, a.align_q, a.align_taps) == (1.5, True, True, 32, 16)
    pairs = [delayed_pair(3000, 2.5, 0.8, 81, True), delayed_pair(2000, 0.0, 0.8, 82), delayed_pair(2500, -4.0, 0.8, 83)]
    xs, ys = [torch.from_numpy(x) for x, _ in pairs], [torch.from_numpy(y) for _, y in pairs]
    ns = argparse.Namespace(align=1.0, align_frac=True, align_polarity=True, align_q=Q, align_taps=W)
    host = dict(device=None, lags=align.host_lags, lags_frac=align.host_lags_frac, shift=align.host_shift)
    al = align.PairAligner(ns, SR, 2, **host)
    assert al.M == 48
    cx, cy = al(xs[:2], ys[:2], ["p0", "p1"])
    cx2, cy2 = al(xs[2:], ys[2:])
    assert al.lag_q == [160, 0, -256] and al.sign == [-1, 1, 1]
    assert al.summary() == "align: lag min = -4  max = 2.5 samples (coded against clean, positive = late), non-zero in 2 of 3 pairs, 1 inverted"
    assert cx[0].shape == cy[0].shape == (3000 - 2 * W + 1,) and rel(cy[0][2 * W:-2 * W], cx[0][2 * W:-2 * W]) < 2e-2
    assert torch.equal(cx[1], xs[1]) and cy[1].data_ptr() == ys[1].data_ptr() and torch.equal(cx2[0], xs[2][4:]) and torch.equal(cy2[0], ys[2][:-4])
    assert capsys.readouterr().err == ""
    # whole samples only: the integer pick, views only; a lag at the edge and an empty support warn on stderr
    ns = argparse.Namespace(align=4000.0 / SR, align_frac=False, align_polarity=False, align_q=Q, align_taps=W)
    al = align.PairAligner(ns, SR, 8, **host)
    assert al.M == 4
    cx, cy = al([xs[2], xs[1]], [ys[2], ys[1][:0]], ["edge", "empty"])
    err = capsys.readouterr().err
    assert al.lag_q == [-4 * Q, 0] and "edge: lag = -4 is at the edge of the search" in err and "empty: the common support" in err and cx[1].numel() == 0
    for bad in (dict(align=None, align_frac=True), dict(align=0.0), dict(align=1e9), dict(align=float("nan")), dict(align=1.0, align_q=1)):
        with pytest.raises(ValueError):
            align.PairAligner(argparse.Namespace(**{**vars(ns), **bad}), SR, 8, **host)
