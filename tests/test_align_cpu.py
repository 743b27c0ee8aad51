"""Alignment in time without a GPU: the host yardsticks of flowdec_amd.align (xcorr against a literal double loop, pick_lag's tie rule,
the common support and its views), the symbols and the refusals of the native entry point that are decided before anything is launched,
and eval_cli --align / enhance_cli --eval-align with the host scorer.

The CLI triple: x = 0.3 s of seeded noise at 48 kHz, x_hat = x delayed by 37 samples plus 1 % noise, y = x advanced by 5 samples plus
30 % noise (a y that IS x after the alignment has a zero noise estimate, and the reference's SI-SDR of that is 0 / 0)."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

from test_eval_cpu import read_csv, write_wav

FD_EINVAL, FD_ENOMEM = -1, -3
SR = 48000
DELAY_H, ADVANCE_Y = 37, 5


def loop_xcorr(a, b, M):
    """The definition, term by term in Python floats (float64)."""
    c = [0.0] * (2 * M + 1)
    for l in range(-M, M + 1):
        for n in range(len(a)):
            if 0 <= n + l < len(b):
                c[l + M] += float(a[n]) * float(b[n + l])
    return np.array(c, np.float64)


def shifted(x, d, length=None):
    """out[n + d] = x[n], zero where nothing lands: x delayed by d samples (advanced for d < 0)."""
    out = np.zeros(len(x) if length is None else length, np.float32)
    for n in range(len(x)):
        if 0 <= n + d < len(out):
            out[n + d] = x[n]
    return out


@pytest.mark.parametrize("La,Lb,M", [(5, 7, 3), (7, 4, 9)])
def test_xcorr_equals_the_double_loop(La, Lb, M):
    from flowdec_amd import align
    rng = np.random.default_rng(La)
    a, b = rng.integers(-9, 10, La).astype(np.float32), rng.integers(-9, 10, Lb).astype(np.float32)
    got, want = align.xcorr(a, b, M), loop_xcorr(a, b, M)
    assert got.dtype == np.float64 and got.shape == (2 * M + 1,) and np.array_equal(got, want)      # small integers: exact in any order
    empty = [l for l in range(-M, M + 1) if min(La, Lb - l) <= max(0, -l)]
    assert (len(empty) > 0) == (M == 9)
    for l in empty:
        assert got[l + M] == 0.0 and not np.signbit(got[l + M])
    assert np.array_equal(align.xcorr(torch.from_numpy(a), torch.from_numpy(b), M), want)
    with pytest.raises(ValueError):
        align.xcorr(a, b, 0)


def test_sign_convention_b_delayed_is_a_positive_lag():
    from flowdec_amd import align
    a = np.array([0, 0, 1, -2, 3, 4, -1, 2, 5, 0, 0], np.float32)        # zeros at both ends: a shift by 2 loses nothing
    for d in (2, -2, 0):
        b = shifted(a, d)
        assert np.dot(a, a) == np.dot(b, b) and align.best_lag(a, b, 3) == d and align.xcorr(a, b, 3)[d + 3] == np.dot(a, a)
    assert align.best_lag(a, shifted(a, 2, length=15), 4) == 2 and align.best_lag(a[:9], shifted(a, 2), 4) == 2


def test_pick_lag_rule():
    from flowdec_amd import align
    nan = float("nan")
    assert align.pick_lag(np.zeros(9)) == 0
    c = np.zeros(9); c[4 - 3] = c[4 + 3] = 2.0
    assert align.pick_lag(c) == 3
    c = np.zeros(9); c[4 + 1] = c[4 - 4] = 2.0
    assert align.pick_lag(c) == 1
    c = np.zeros(9); c[4 - 1] = c[4 + 1] = 2.0; c[4 + 4] = 2.0
    assert align.pick_lag(c) == 1
    assert align.pick_lag([nan, 1.0, nan, 0.5, nan]) == -1            # NaN entries are ignored
    assert align.pick_lag([nan, -3.0, nan, -5.0, nan]) == -1
    assert align.pick_lag([nan] * 7) == 0
    assert align.pick_lag([-math.inf, nan, -math.inf]) == 0
    assert align.pick_lag([5.0, 1.0, 1.0]) == -1 and isinstance(align.pick_lag([5.0, 1.0, 1.0]), int)
    with pytest.raises(ValueError):
        align.pick_lag([1.0, 2.0])


@pytest.mark.parametrize("Lx,Lh,Ly,lag_h,lag_y,want", [
    (100, 100, 100, 7, -3, (3, 93)),        # n0 from -lag_y, n1 from Lh - lag_h
    (100, 100, 100, -7, 3, (7, 97)),        # n0 from -lag_h, n1 from Ly - lag_y
    (50, 100, 100, 7, 3, (0, 50)),          # n0 = 0, n1 from Lx
    (100, 60, 200, -2, 5, (2, 62)),         # n1 from Lh - lag_h with a negative lag
    (100, 200, 40, 0, -10, (10, 50)),       # n1 from Ly - lag_y
    (100, 30, 100, 30, 0, (0, 0)),          # empty: x_hat starts where it ends
    (20, 100, 100, 0, -25, (25, 20)),       # empty: n1 < n0
])
def test_common_support_and_views(Lx, Lh, Ly, lag_h, lag_y, want):
    from flowdec_amd import align
    assert align.common_support(Lx, Lh, Ly, lag_h, lag_y) == want
    h, x, y = torch.arange(Lh, dtype=torch.float32), torch.arange(Lx, dtype=torch.float32) + 1000, torch.arange(Ly, dtype=torch.float32) + 5000
    ah, ax, ay = align.align_triple(h, x, y, lag_h, lag_y)
    n0, n1 = want
    n = max(n1 - n0, 0)
    assert ah.shape == ax.shape == ay.shape == (n,)
    if n:
        assert ah.data_ptr() == h.data_ptr() + 4 * (n0 + lag_h) and ax.data_ptr() == x.data_ptr() + 4 * n0 and ay.data_ptr() == y.data_ptr() + 4 * (n0 + lag_y)
        assert torch.equal(ah, h[n0 + lag_h:n1 + lag_h]) and torch.equal(ax, x[n0:n1]) and torch.equal(ay, y[n0 + lag_y:n1 + lag_y])
        assert ah[0] == n0 + lag_h and ax[0] == 1000 + n0 and ay[-1] == 5000 + n1 + lag_y - 1
    # NumPy arrays come back as views too
    nh, nx, ny = align.align_triple(h.numpy(), x.numpy(), y.numpy(), lag_h, lag_y)
    assert nh.shape == nx.shape == ny.shape == (n,) and (n == 0 or (nh.base is not None and np.shares_memory(nx, x.numpy())))


def test_host_lags_and_module_layering():
    import subprocess
    import sys
    from conftest import ROOT
    from flowdec_amd import align
    rng = np.random.default_rng(3)
    a = [rng.standard_normal(n).astype(np.float32) for n in (300, 411)]
    b = [shifted(a[0], 9, length=320), shifted(a[1], -4, length=400)]
    lags, cs = align.host_lags(a, b, 12, batch=2, return_xcorr=True)
    assert lags.dtype == np.int64 and lags.tolist() == [9, -4] and cs.shape == (2, 25) and np.array_equal(cs[1], align.xcorr(a[1], b[1], 12))
    assert align.host_lags(a, b, 12).tolist() == [9, -4] and align.host_lags([], [], 3).shape == (0,)
    with pytest.raises(ValueError):
        align.host_lags(a, b[:1], 12)
    with pytest.raises(ValueError):
        align.lags_batch(a, b, (1 << 20) + 1)
    code = ("import sys, torch, flowdec_amd.align, flowdec_amd._lib as L\n"
            "print(sorted(k for k in sys.modules if k.startswith('flowdec_amd.') and k.endswith('_cli')), L._lib is None, torch.cuda.is_initialized())\n")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().splitlines()[-1] == "[] True False", r.stdout + r.stderr[-2000:]


def test_symbols_and_refusals_without_a_gpu():
    import __graft_entry__ as g
    g.build()
    from flowdec_amd import _lib
    lib = _lib.load()
    src = open(os.path.join(g.ROOT, "include", "flowdec_hip.h")).read()
    for name in ("fd_xcorr_workspace_bytes", "fd_xcorr_lags"):
        assert name + "(" in src and hasattr(lib, name) and name in _lib.SIGNATURES
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
    assert "xcorr.hip" in __import__("flowdec_amd.build", fromlist=["SOURCES"]).SOURCES
    err = lambda: lib.fd_last_error().decode()
    p = C.c_void_p(16)                       # never dereferenced: every call below refuses before a launch
    big, cap, row = 1 << 40, 1 << 20, 0x7fffffff - 1024
    call = lambda a=p, b=p, la=p, lb=p, B=2, La=1000, Lb=900, M=300, c=p, lags=p, ws=p, n=big: lib.fd_xcorr_lags(a, b, la, lb, B, La, Lb, M, c, lags, ws, n, None)
    for kw in (dict(a=None), dict(b=None), dict(la=None), dict(lb=None), dict(lags=None), dict(ws=None)):
        assert call(**kw) == FD_EINVAL and "fd_xcorr_lags: null pointer" in err()
    for kw, word in ((dict(B=0), "B 0"), (dict(B=65536), "B 65536"), (dict(B=-1), "B -1"), (dict(M=0), "max_lag 0"), (dict(M=cap + 1), "max_lag"),
                     (dict(M=-5), "max_lag -5"), (dict(La=0), "La 0"), (dict(Lb=0), "Lb 0"), (dict(La=-3), "La -3"), (dict(La=row + 1), "row lengths"),
                     (dict(Lb=row + 1), "row lengths")):
        assert call(c=None, **kw) == FD_EINVAL and "fd_xcorr_lags" in err() and word in err(), (kw, err())
    need = lib.fd_xcorr_workspace_bytes(2, 1000, 900, 300)
    assert need >= 2 * 601 * 8
    for c in (p, None):
        assert call(c=c, n=need - 1) == FD_ENOMEM and "fd_xcorr_lags" in err() and "workspace" in err()
        assert call(c=c, n=0) == FD_ENOMEM
    # the size: 0 for every bad argument, grows with the batch, the search and the rows of a; the largest call is refused by nothing
    for bad in ((0, 1000, 900, 300), (65536, 1000, 900, 300), (2, 0, 900, 300), (2, 1000, 0, 300), (2, 1000, 900, 0), (2, 1000, 900, cap + 1),
                (2, row + 1, 900, 300), (2, 1000, row + 1, 300), (-1, 1000, 900, 300)):
        assert lib.fd_xcorr_workspace_bytes(*bad) == 0, bad
    assert need < lib.fd_xcorr_workspace_bytes(4, 1000, 900, 300) and need < lib.fd_xcorr_workspace_bytes(2, 1000, 900, 600)
    assert need < lib.fd_xcorr_workspace_bytes(2, 100000, 900, 300) and need == lib.fd_xcorr_workspace_bytes(2, 1000, 5000, 300)
    assert lib.fd_xcorr_workspace_bytes(65535, row, row, cap) > 0


def cli_signals(n=int(0.3 * SR), seed=11, delay_h=DELAY_H, advance_y=ADVANCE_Y):
    rng = np.random.default_rng(seed)
    x = (0.1 * rng.standard_normal(n)).astype(np.float32)
    h = shifted(x, delay_h) + (0.001 * rng.standard_normal(n)).astype(np.float32)
    y = shifted(x, -advance_y) + (0.03 * rng.standard_normal(n)).astype(np.float32)
    return h, x, y


def make_delayed_triples(tmp_path, specs=((int(0.3 * SR), 11, DELAY_H, ADVANCE_Y),)):
    """One `clean ---> noisy ---> enhanced` line per (n, seed, delay of x_hat, advance of y); float32 wav files at 48 kHz."""
    lines = []
    for i, (n, seed, dh, ay) in enumerate(specs):
        h, x, y = cli_signals(n, seed, dh, ay)
        paths = [tmp_path / f"clean_{i}.wav", tmp_path / f"noisy_{i}.wav", tmp_path / f"enh_{i}.wav"]
        for path, s in zip(paths, (x, y, h)):
            write_wav(path, s, SR)
        lines.append(" ---> ".join(str(q) for q in paths))
    lst = tmp_path / "triples_list.txt"
    lst.write_text("\n".join(lines) + "\n")
    return lst


def test_eval_cli_align_on_the_host_scorer(tmp_path, capsys):
    from flowdec_amd import eval_cli
    lst = make_delayed_triples(tmp_path)
    out = {k: tmp_path / f"{k}.csv" for k in ("plain", "align", "all", "crop")}
    flags = dict(plain=[], align=["--align", "2"], all=["--estoi", "--spectral", "--align", "2"], crop=["--align", "2", "--crop-to-x", "--crop-to-x-hat"])
    res, caps, heads, rows = {}, {}, {}, {}
    for k in out:
        res[k] = eval_cli.run(["--triples", str(lst), "--out", str(out[k])] + flags[k], scorer=eval_cli.HOST_SCORER)
        caps[k] = capsys.readouterr()
        heads[k], rows[k] = read_csv(out[k])
    assert tuple(heads["plain"]) == eval_cli.CSV_HEADER and res["plain"].lags == []
    assert float(rows["plain"][0][4]) < 0.0                                      # misaligned white noise: SI-SDR below 0 dB
    assert tuple(heads["align"]) == eval_cli.CSV_HEADER + ("lag_x_hat", "lag_y") == eval_cli.CSV_HEADER + eval_cli.LAG_NAMES
    assert rows["align"][0][-2:] == [str(DELAY_H), str(-ADVANCE_Y)]
    assert float(rows["align"][0][4]) > 35.0 and all(math.isfinite(float(v)) for v in rows["align"][0][4:8])
    assert tuple(heads["all"]) == eval_cli.CSV_HEADER + ("estoi", "msstft", "mel", "lag_x_hat", "lag_y")
    assert rows["all"][0][-2:] == [str(DELAY_H), str(-ADVANCE_Y)] and rows["all"][0][:8] == rows["align"][0][:8]
    assert rows["crop"] == rows["align"] and heads["crop"] == heads["align"]      # the crop flags find nothing to cut
    # the summary: the means as before, then one line per lag column with min, max and the count of non-zero lags
    assert res["align"].lags == [("lag_x_hat", DELAY_H, DELAY_H, 1), ("lag_y", -ADVANCE_Y, -ADVANCE_Y, 1)]
    assert caps["align"].out.count("mean =") == 4 and caps["all"].out.count("mean =") == 7 and "lag_x_hat" not in caps["plain"].out
    assert f"min = {DELAY_H}  max = {DELAY_H}  non-zero in 1 of 1" in caps["align"].out and f"min = {-ADVANCE_Y}" in caps["align"].out
    assert "edge of the search" not in caps["align"].err
    # the aligned triple is scored exactly as files cut by hand to the common support
    h, x, y = (eval_cli.load_mono(rows["plain"][0][k], SR) for k in (1, 2, 3))
    n0, n1 = 5, len(x) - DELAY_H
    want = eval_cli.score([(h[n0 + DELAY_H:n1 + DELAY_H], x[n0:n1], y[n0 - ADVANCE_Y:n1 - ADVANCE_Y])], SR, 8, eval_cli.HOST_SCORER)
    assert [float(v) for v in rows["align"][0][4:8]] == want[0].tolist()


def test_without_align_nothing_changes_and_the_scorer_is_not_asked(tmp_path, capsys):
    from flowdec_amd import eval_cli
    lst = make_delayed_triples(tmp_path)

    def boom(*a, **k):
        raise AssertionError("Scorer.align was called without --align")

    H = eval_cli.HOST_SCORER
    assert eval_cli.Scorer(H.si_sxr, H.logspec).align is None and eval_cli.Scorer(H.si_sxr, H.logspec, H.estoi, H.spectral).align is None
    assert eval_cli.GPU_SCORER.align is not None and H.align is not None
    trap = eval_cli.Scorer(H.si_sxr, H.logspec, H.estoi, H.spectral, boom)
    for flags in ([], ["--estoi", "--spectral"], ["--crop-to-x"]):
        eval_cli.run(["--triples", str(lst), "--out", str(tmp_path / "a.csv")] + flags, scorer=trap)
        a = capsys.readouterr()
        eval_cli.run(["--triples", str(lst), "--out", str(tmp_path / "b.csv")] + flags, scorer=eval_cli.Scorer(H.si_sxr, H.logspec, H.estoi, H.spectral))
        b = capsys.readouterr()
        assert (tmp_path / "a.csv").read_bytes() == (tmp_path / "b.csv").read_bytes()
        assert a.out.replace("a.csv", "b.csv") == b.out and "lag" not in a.out
    assert tuple(read_csv(tmp_path / "a.csv")[0]) == eval_cli.CSV_HEADER
    # with --align the trap springs, and a scorer without the field refuses like estoi does
    with pytest.raises(AssertionError):
        eval_cli.run(["--triples", str(lst), "--out", str(tmp_path / "c.csv"), "--align", "2"], scorer=trap)
    with pytest.raises(ValueError):
        eval_cli.run(["--triples", str(lst), "--out", str(tmp_path / "c.csv"), "--align", "2"], scorer=eval_cli.Scorer(H.si_sxr, H.logspec))
    assert eval_cli.build_parser().parse_args(["--triples", "t", "--out", "o"]).align is None


def test_edge_warning_empty_support_and_parser_errors(tmp_path, capsys):
    from flowdec_amd import eval_cli
    lst = make_delayed_triples(tmp_path)
    ms = DELAY_H * 1000.0 / SR                                                   # M = 37: the peak of x_hat sits on the edge
    assert eval_cli.align_max_lag(ms, SR) == DELAY_H and eval_cli.align_max_lag(2, SR) == 96 and eval_cli.align_max_lag(100, 16000) == 1600
    eval_cli.run(["--triples", str(lst), "--out", str(tmp_path / "e.csv"), "--align", repr(ms)], scorer=eval_cli.HOST_SCORER)
    cap = capsys.readouterr()
    head, rows = read_csv(tmp_path / "e.csv")
    assert rows[0][-2:] == [str(DELAY_H), str(-ADVANCE_Y)] and float(rows[0][4]) > 35.0                # still scored
    assert cap.err.count("edge of the search") == 1 and "lag_x_hat = 37" in cap.err and "enh_0.wav" in cap.err
    for bad in ("0", "-1", "0.005", "nan", str(((1 << 20) + 1) * 1000.0 / SR)):
        with pytest.raises(SystemExit) as e:
            eval_cli.run(["--triples", str(lst), "--out", str(tmp_path / "p.csv"), "--align", bad], scorer=eval_cli.HOST_SCORER)
        assert e.value.code == 2
        assert "--align" in capsys.readouterr().err
    assert not (tmp_path / "p.csv").exists()
    # an empty common support: a warning, NaN in every metric, the lags still written
    H = eval_cli.HOST_SCORER
    far = eval_cli.Scorer(H.si_sxr, H.logspec, H.estoi, H.spectral, lambda as_, bs, M, batch: np.array([len(as_[0]), 0], np.int64))
    eval_cli.run(["--triples", str(lst), "--out", str(tmp_path / "f.csv"), "--align", "2"], scorer=far)
    cap = capsys.readouterr()
    head, rows = read_csv(tmp_path / "f.csv")
    assert rows[0][4:8] == ["nan"] * 4 and rows[0][-2:] == [str(int(0.3 * SR)), "0"] and "common support" in cap.err and "empty" in cap.err


def test_eval_align_reaches_eval_cli(monkeypatch):
    from flowdec_amd import enhance_cli, eval_cli
    base = ["--ckpt", "c", "--files", "f", "--outdir", "o", "--N", "3"]
    assert enhance_cli.build_parser().parse_args(base + ["--eval"]).eval_align is None
    args = enhance_cli.build_parser().parse_args(base + ["--eval", "--eval-align", "2.5"])
    assert args.eval and args.eval_align == 2.5 and not args.eval_spectral
    seen = []
    monkeypatch.setattr(eval_cli, "run", lambda argv, **kw: seen.append(list(argv)))
    monkeypatch.setattr(torch.cuda, "device", lambda d: __import__("contextlib").nullcontext())
    args.device, args.batch_files = "cuda", 4
    enhance_cli.evaluate_triples(args, "")
    args.eval_spectral = True
    enhance_cli.evaluate_triples(args, "")
    args.eval_align = None
    enhance_cli.evaluate_triples(args, "")
    assert seen[0][-2:] == ["--align", "2.5"] and seen[1][-3:] == ["--spectral", "--align", "2.5"] and seen[2][-1] == "--spectral"
    assert seen[0][:-2] == seen[2][:-1]
    assert eval_cli.build_parser().parse_args(seen[1]).align == 2.5
