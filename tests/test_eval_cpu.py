"""flowdec_amd/eval_cli.py and the host side of the GPU metrics (flowdec_amd/metrics.py), without a GPU: triples parsing, the crop rules
and their order, the NaN row of unequal lengths, the CSV's header and row order, the summary, the dB values formed from the two-pass
float64 sums of fd_metrics_sisxr, and the --eval flag of enhance_cli.  The scorer here is eval_cli.HOST_SCORER (the host functions of
metrics.py); the GPU scorer is tested in tests/test_hip_metrics.py."""
import csv
import math
import os

import numpy as np
import pytest
import torch

from conftest import load_golden


def write_wav(path, x, sr=48000):
    from flowdec_amd.enhance_cli import save_wav
    save_wav(str(path), torch.as_tensor(np.asarray(x, np.float32)), sr)


def two_pass_sums(x_hat, x, y):
    """NumPy float64 restatement of what fd_metrics_sisxr accumulates (include/flowdec_hip.h "Evaluation metrics"), in its layout."""
    h, x, y = (np.asarray(a, np.float32).astype(np.float64) for a in (x_hat, x, y))
    xy, xx, hx = np.dot(x, y), np.dot(x, x), np.dot(h, x)
    n = y + x if xy < 0 else y - x
    hn, nn = np.dot(h, n), np.dot(n, n)
    st, en = (hx / xx) * x, (hn / nn) * n
    ea = h - st - en
    return np.array([xx, hx, hn, nn, np.dot(st, st), np.dot(en, en), np.dot(ea, ea), np.dot(en + ea, en + ea)])


def test_read_triples_and_commas(tmp_path):
    from flowdec_amd import eval_cli
    lst = tmp_path / "triples_list.txt"
    lst.write_text("/a/clean 1.wav ---> /b/noisy,take 2.wav ---> /c/out,take 2.wav\n\n  /a/c2.wav ---> /b/n2.wav ---> /c/n2.wav  \n")
    t = eval_cli.read_triples(str(lst))
    assert [(v.x, v.y, v.x_hat) for v in t] == [("/a/clean 1.wav", "/b/noisy,take 2.wav", "/c/out,take 2.wav"), ("/a/c2.wav", "/b/n2.wav", "/c/n2.wav")]
    assert [v.name for v in t] == ["out,take 2.wav", "n2.wav"]
    lst.write_text("/a/c.wav ---> /b/n.wav\n")
    with pytest.raises(ValueError, match=r"triples_list.txt:1: 2 fields"):
        eval_cli.read_triples(str(lst))


def test_crop_rules_and_their_order():
    from flowdec_amd.eval_cli import crop
    h, x, y = torch.arange(12.0), torch.arange(10.0), torch.arange(11.0)
    assert [int(v.numel()) for v in crop(h, x, y, False, False)] == [12, 10, 11]
    assert [int(v.numel()) for v in crop(h, x, y, True, False)] == [10, 10, 10]
    assert [int(v.numel()) for v in crop(h, x, y, False, True)] == [12, 10, 11]       # x is shorter than x_hat: only y could be cut, and is not longer
    h2 = torch.arange(8.0)
    assert [int(v.numel()) for v in crop(h2, x, y, False, True)] == [8, 8, 8]
    # the order matters when x_hat is the longest and y the shortest: crop-to-x first, then crop-to-x-hat (which is then x's length)
    h3, x3, y3 = torch.arange(12.0), torch.arange(10.0), torch.arange(9.0)
    assert [int(v.numel()) for v in crop(h3, x3, y3, True, True)] == [10, 10, 9]
    assert torch.equal(crop(h, x, y, True, False)[0], h[:10])


def make_corpus(tmp_path, lengths, sr=48000, seed=0):
    rng = np.random.default_rng(seed)
    lines, sigs = [], []
    for i, (lh, lx, ly) in enumerate(lengths):
        x = 0.1 * rng.standard_normal(max(lh, lx, ly)).astype(np.float32)
        y = x + 0.05 * rng.standard_normal(len(x)).astype(np.float32)
        h = x + 0.01 * rng.standard_normal(len(x)).astype(np.float32)
        paths = [tmp_path / f"clean_{i}.wav", tmp_path / f"noisy_{i}.wav", tmp_path / f"enh_{i}.wav"]
        for p, s, l in zip(paths, (x, y, h), (lx, ly, lh)):
            write_wav(p, s[:l], sr)
        lines.append(" ---> ".join(str(p) for p in paths))
        sigs.append((h[:lh], x[:lx], y[:ly]))
    lst = tmp_path / "triples_list.txt"
    lst.write_text("\n".join(lines) + "\n")
    return lst, sigs


def read_csv(path):
    with open(path, newline="") as f:
        rows = list(csv.reader(f))
    return rows[0], rows[1:]


def test_csv_rows_in_list_order_nan_row_and_summary(tmp_path, capsys):
    from flowdec_amd import eval_cli, metrics
    # lengths out of order so that length-sorted batches of 2 reorder them; triple 2 has unequal lengths
    lengths = [(6000, 6000, 6000), (2000, 2000, 2000), (3100, 3000, 3000), (4000, 4000, 4000), (1000, 1000, 1000)]
    lst, sigs = make_corpus(tmp_path, lengths)
    assert [b for b in metrics.length_sorted_batches([l[1] for l in lengths], 2)] == [[4, 1], [2, 3], [0]]
    out = tmp_path / "sub" / "metrics.csv"
    res = eval_cli.run(["--triples", str(lst), "--out", str(out), "--batch-files", "2"], scorer=eval_cli.HOST_SCORER)
    assert res.exit_code == 0 and res.n_triples == 5 and res.n_scored == 5 and res.n_unreadable == 0
    header, rows = read_csv(out)
    assert header == ["name", "x_hat", "x", "y", "sisdr", "sisir", "sisar", "logspec_mse"]
    assert [r[0] for r in rows] == [f"enh_{i}.wav" for i in range(5)]
    assert [r[1:4] for r in rows] == [[str(tmp_path / f"enh_{i}.wav"), str(tmp_path / f"clean_{i}.wav"), str(tmp_path / f"noisy_{i}.wav")] for i in range(5)]
    vals = np.array([[float(v) for v in r[4:]] for r in rows])
    assert np.isnan(vals[2]).all() and np.isfinite(np.delete(vals, 2, axis=0)).all()
    for i in (0, 1, 3, 4):
        np.testing.assert_allclose(vals[i, :3], metrics.si_sxr(*sigs[i]), rtol=0, atol=1e-9)
        assert vals[i, 3] == metrics.logspec_mse(sigs[i][0], sigs[i][1])
    # the summary skips the NaN row
    assert [m[0] for m in res.means] == list(eval_cli.METRIC_NAMES) and all(m[2] == 4 for m in res.means)
    np.testing.assert_allclose([m[1] for m in res.means], np.delete(vals, 2, axis=0).mean(axis=0), rtol=1e-12)
    cap = capsys.readouterr()
    assert "enh_2.wav: lengths differ" in cap.err and "over 4 finite rows" in cap.out
    # with --crop-to-x the same triple is scored
    res = eval_cli.run(["--triples", str(lst), "--out", str(out), "--crop-to-x"], scorer=eval_cli.HOST_SCORER)
    _, rows = read_csv(out)
    np.testing.assert_allclose([float(v) for v in rows[2][4:7]], metrics.si_sxr(sigs[2][0][:3000], sigs[2][1][:3000], sigs[2][2][:3000]), atol=1e-9)
    assert all(m[2] == 5 for m in res.means)


def test_summary_of_nothing_and_all_nan():
    from flowdec_amd.eval_cli import summary
    s = summary(np.full((2, 4), np.nan))
    assert all(math.isnan(m[1]) and m[2] == 0 for m in s)
    s = summary(np.array([[1.0, 2.0, np.inf, np.nan], [3.0, np.nan, 5.0, 7.0]]))
    assert [(m[1], m[2]) for m in s] == [(2.0, 2), (2.0, 1), (5.0, 1), (7.0, 1)]


def test_unreadable_triple_is_skipped_and_counted_and_short_clip_has_nan_spectral(tmp_path, capsys):
    from flowdec_amd import eval_cli
    lst, _ = make_corpus(tmp_path, [(2000, 2000, 2000), (500, 500, 500), (2500, 2500, 2500)])
    os.remove(tmp_path / "noisy_2.wav")
    out = tmp_path / "metrics.csv"
    res = eval_cli.run(["--triples", str(lst), "--out", str(out)], scorer=eval_cli.HOST_SCORER)
    assert res.exit_code == 3 and res.n_unreadable == 1 and res.n_scored == 2
    _, rows = read_csv(out)
    assert [r[0] for r in rows] == ["enh_0.wav", "enh_1.wav"]
    assert rows[1][7] == "nan" and all(math.isfinite(float(v)) for v in rows[1][4:7])       # 500 samples < 769: SI-SxR only
    assert "too few for the spectral metric" in capsys.readouterr().err


def test_load_mono_means_channels_and_resamples(tmp_path):
    from flowdec_amd import eval_cli
    from flowdec_amd.enhance_cli import resample, resampled_length
    rng = np.random.default_rng(3)
    st = (0.1 * rng.standard_normal((2, 4410))).astype(np.float32)
    write_wav(tmp_path / "st.wav", st, 44100)
    got = eval_cli.load_mono(str(tmp_path / "st.wav"), 48000)
    assert got.ndim == 1 and got.numel() == resampled_length(4410, 44100, 48000) == 4800
    want = resample(torch.from_numpy(st).mean(dim=0, keepdim=True), 44100, 48000, lowpass_filter_width=256)[0]
    assert torch.equal(got, want)
    assert torch.equal(eval_cli.load_mono(str(tmp_path / "st.wav"), 44100), torch.from_numpy(st).mean(dim=0))


def test_db_values_from_two_pass_sums_match_host_and_golden():
    """The float64 two-pass algorithm of the kernel, restated in NumPy, through metrics.sisxr_from_sums: equal to metrics.si_sxr and to the
    reference's values of g14 within the tolerance of the host test (1e-4 dB), the phase-flipped case included."""
    from flowdec_amd import metrics
    g = load_golden("g14_metrics.npz")
    flips = 0
    for i in range(3):
        h, x, y = g[f"xhat{i}"], g[f"x{i}"], g[f"y{i}"]
        flips += float(np.dot(x.astype(np.float64), y.astype(np.float64))) < 0
        got = metrics.sisxr_from_sums(two_pass_sums(h, x, y))
        assert got.shape == (1, 3)
        np.testing.assert_allclose(got[0], metrics.si_sxr(h, x, y), rtol=0, atol=1e-4)
        np.testing.assert_allclose(got[0], g[f"sisxr{i}"], rtol=0, atol=1e-4)
    assert flips >= 1
    assert len(metrics.SISXR_SUMS) == 8
    # a zero residual is +inf dB, not an error
    s = np.array([[1.0, 1.0, 0.0, 1.0, 1.0, 0.0, 0.0, 0.0]])
    assert np.isposinf(metrics.sisxr_from_sums(s)).all()


def test_batch_functions_refuse_bad_input_before_touching_the_gpu():
    from flowdec_amd import metrics
    a, b = torch.zeros(100), torch.zeros(99)
    with pytest.raises(ValueError, match="differ in length"):
        metrics.si_sxr_batch([a], [b], [a])
    with pytest.raises(ValueError, match="one entry per clip"):
        metrics.si_sxr_batch([a, a], [a], [a])
    with pytest.raises(ValueError, match="768"):
        metrics.logspec_mse_batch([torch.zeros(768)], [torch.zeros(768)])


def test_enhance_cli_parser_has_eval_off_by_default():
    from flowdec_amd.enhance_cli import build_parser
    base = ["--ckpt", "c", "--files", "f", "--outdir", "o", "--N", "3"]
    assert build_parser().parse_args(base).eval is False
    assert build_parser().parse_args(base + ["--eval"]).eval is True


def test_metrics_symbols_are_declared_exported_and_bound():
    import ctypes as C
    from conftest import ROOT
    from flowdec_amd import _lib as L
    lib = L.load()
    src = open(os.path.join(ROOT, "include", "flowdec_hip.h")).read()
    for name in ("fd_metrics_workspace_bytes", "fd_metrics_sisxr", "fd_metrics_logspec_mse", "fd_metrics_power_spec"):
        assert name + "(" in src and name in L.SIGNATURES and hasattr(lib, name)
    # host-only: sizes grow with the batch, the spectral part dominates, bad shapes give 0
    a, b = lib.fd_metrics_workspace_bytes(1, 4000, 0, 0), lib.fd_metrics_workspace_bytes(4, 4000, 0, 0)
    assert 0 < a < b < lib.fd_metrics_workspace_bytes(4, 4000, 1536, 384)
    assert lib.fd_metrics_workspace_bytes(4, 4000, 1536, 384) >= 3 * 4 * 11 * 1664 * 4
    assert lib.fd_metrics_workspace_bytes(0, 4000, 1536, 384) == 0 and lib.fd_metrics_workspace_bytes(1, 0, 1536, 384) == 0
    # refusals need no GPU: they return before any launch
    assert lib.fd_metrics_sisxr(None, None, None, None, 1, 10, None, None, 0, None) == -1 and b"null pointer" in lib.fd_last_error()
    one = C.c_void_p(16)
    assert lib.fd_metrics_sisxr(one, one, one, one, 1, 10, one, one, 8, None) == -1 and b"workspace too small" in lib.fd_last_error()
