"""ESTOI without a GPU: the host function flowdec_amd.metrics.estoi (NumPy float64, the yardstick of csrc/stoi.hip), its resampling
bank, eval_cli --estoi with the host scorer, and the refusals of the native entry points that are decided before anything is launched.

What is pinned here: the 10 kHz bank against scipy.signal.resample_poly with pystoi's window, the band edges, the frame arithmetic and the
properties of the metric.  Parity with the pystoi package itself is NOT pinned (it is not installed; scripts/pin_estoi.py prints it where
it is).

The bound of the bank test.  fd_resample's loop (include/flowdec_hip.h "Resampling") forms output m as a float64 sum of exact products
bank[i][k] x[j] with the bank rounded ONCE from float64 to float32: every tap is off by at most u32 |tap|, u32 = 2^-24, so the output by at
most u32 sum_j |p w x[j]| = u32 A_m, A_m = resample_poly(|x|, p, q, window = |w|)[m].  Both float64 summations (here and in SciPy, K
terms) add at most 2 K u64 A_m, u64 = 2^-53, which K <= 1741 keeps below 4e-13 A_m; it is included."""
import csv
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

from test_eval_cpu import read_csv, write_wav

EDGES = [(7, 9), (9, 11), (11, 14), (14, 17), (17, 22), (22, 27), (27, 34), (34, 43), (43, 55), (55, 69), (69, 87), (87, 109), (109, 138), (138, 174),
         (174, 219)]
FD_EINVAL = -1


def gated_clip(sr, dur, seed):
    """Seeded white noise under a slow envelope with a gate (80 dB down when closed): the 40 dB mask removes frames in the middle of the
    clip, so kept frames are not adjacent at the source.  float32."""
    rng = np.random.default_rng(seed)
    n = int(round(sr * dur))
    t = np.arange(n) / sr
    env = 0.55 + 0.45 * np.sin(2 * np.pi * 3 * t)
    gate = (np.sin(2 * np.pi * 2.3 * t + 0.3) > -0.8).astype(np.float64)
    return (0.2 * rng.standard_normal(n) * env * (gate + 1e-4)).astype(np.float32)


def noisy(x, snr_db, seed):
    rng = np.random.default_rng(seed)
    nz = rng.standard_normal(len(x))
    nz *= np.sqrt(np.mean(x.astype(np.float64) ** 2) / np.mean(nz ** 2)) * 10 ** (-snr_db / 20)
    return (x + nz).astype(np.float32)


@pytest.mark.parametrize("sr,o,n,width,L", [(16000, 8, 5, 58, 290), (48000, 24, 5, 174, 870), (44100, 441, 100, None, None)])
def test_bank_equals_scipy_resample_poly(sr, o, n, width, L):
    signal = pytest.importorskip("scipy.signal")
    from flowdec_amd import metrics
    w, p, q, Lf = metrics.estoi_filter(sr)
    bank, bo, bn, bw = metrics.estoi_bank(sr)
    assert (bo, bn) == (o, n) == (q, p) and bank.dtype == np.float32 and bank.shape == (n, 2 * bw + o)
    assert bw == -(-Lf // p) and len(w) == 2 * Lf + 1 and abs(np.sum(w) - 1) < 1e-12
    if width is not None:
        assert (bw, Lf) == (width, L)
    if sr == 44100:
        assert bank.shape[1] == 761
    assert n * bank.shape[1] <= 1 << 24
    x = np.random.default_rng(sr).standard_normal(3001).astype(np.float32).astype(np.float64)
    ref = signal.resample_poly(x, p, q, window=w)
    got = metrics.polyphase_resample(x, bank, bo, bn, bw)
    assert len(got) == len(ref) == -(-p * 3001 // q)                        # the output length is SciPy's
    A = signal.resample_poly(np.abs(x), p, q, window=np.abs(w))
    bound = (2.0 ** -24 + 2 * len(w) * 2.0 ** -53) * A
    err = np.abs(got - ref)
    print(f"sr {sr}: max err {err.max():.3g} at outputs up to {np.abs(ref).max():.3g}, max err / bound {np.max(err / bound):.3g}")
    assert (err <= bound).all()
    # the float64 bank of the host function is SciPy's arithmetic up to the order of summation
    b64 = metrics._estoi_bank64(sr)[0]
    assert np.abs(metrics.polyphase_resample(x, b64, bo, bn, bw) - ref).max() <= 2 * len(w) * 2.0 ** -53 * A.max()


def test_band_edges_and_frame_arithmetic():
    from flowdec_amd import metrics
    assert metrics.estoi_band_edges() == EDGES
    assert metrics.ESTOI_EPS == np.finfo(float).eps == 2.0 ** -52
    x = gated_clip(48000, 1.0, 0)
    d = metrics.estoi_detail(x, x, 48000)
    # 48000 samples -> 10000 at 10 kHz -> range(0, 9744, 128): 77 frames; the gate closes twice in this clip and takes ten of them
    assert d["frames"] == 77 == len(range(0, 10000 - 256, 128))
    assert len(d["kept"]) == 67 and d["spectral_frames"] == 66 and d["tob_x"].shape == (66, 15)
    assert np.any(np.diff(d["kept"]) > 1) and not d["too_short"]
    # the frame that would end exactly at the signal's end is not taken (pystoi's loop)
    assert metrics.estoi_detail(np.ones(256 + 128), np.ones(256 + 128), 10000)["frames"] == 1
    assert metrics.estoi_detail(np.ones(256 + 129), np.ones(256 + 129), 10000)["frames"] == 2
    assert metrics.estoi_detail(np.ones(256), np.ones(256), 10000)["frames"] == 0


def test_host_function_properties():
    from flowdec_amd import metrics
    x = gated_clip(48000, 1.0, 0)
    assert abs(metrics.estoi(x, x, 48000) - 1.0) < 1e-12
    vals = [metrics.estoi(noisy(x, snr, 1), x, 48000) for snr in (20, 5, -5)]
    print("estoi at 20 / 5 / -5 dB:", vals)
    assert 1.0 > vals[0] > vals[1] > vals[2] > 0.0 and vals[0] > 0.9 and vals[2] < 0.5
    y = noisy(x, 5, 2)
    assert metrics.estoi(4 * y, x, 48000) == metrics.estoi(y, x, 48000)       # a power of two commutes with every rounding; the mask reads x only
    # the float32 mode rounds where the kernels round: close to, and not the same as, the float64 value
    a, b = metrics.estoi(y, x, 48000), metrics.estoi(y, x, 48000, precision="float32")
    assert 0 < abs(a - b) < 1e-6
    # 0.4 s: 30 frames, fewer than 30 spectral frames
    short = metrics.estoi_detail(y[:19200], x[:19200], 48000)
    assert short["value"] == 1e-5 == metrics.ESTOI_TOO_SHORT and short["too_short"] and short["spectral_frames"] < 30
    assert metrics.estoi(x[:100], x[:100], 48000) == 1e-5
    with pytest.raises(ValueError, match="differ in length"):
        metrics.estoi(x[:-1], x, 48000)
    # 10 kHz input is not resampled; 16 kHz goes through its own bank
    x10 = gated_clip(10000, 1.0, 3)
    assert abs(metrics.estoi(x10, x10, 10000) - 1.0) < 1e-12
    x16 = gated_clip(16000, 1.0, 4)
    assert 0.2 < metrics.estoi(noisy(x16, 5, 5), x16, 16000) < 0.95


def test_zero_row_in_estimate_is_finite():
    """A band that is exactly zero in every frame of x_hat (here: x_hat = 0) normalises to zeros: the one deliberate deviation from pystoi."""
    from flowdec_amd import metrics
    x = gated_clip(10000, 1.0, 6)
    v = metrics.estoi(np.zeros_like(x), x, 10000)
    assert v == 0.0
    # a pure low tone leaves the upper bands of x_hat at rounding noise or zero; the result stays finite
    t = np.arange(len(x)) / 10000
    assert math.isfinite(metrics.estoi(np.sin(2 * np.pi * 200 * t).astype(np.float32), x, 10000))


def make_triples(tmp_path, durs, sr=16000, seed=0, snr=5):
    lines, sigs = [], []
    for i, d in enumerate(durs):
        x = gated_clip(sr, d, seed + 10 * i)
        y, h = noisy(x, snr - 5, seed + 10 * i + 1), noisy(x, snr + 3 * i, seed + 10 * i + 2)
        paths = [tmp_path / f"clean_{i}.wav", tmp_path / f"noisy_{i}.wav", tmp_path / f"enh_{i}.wav"]
        for p, s in zip(paths, (x, y, h)):
            write_wav(p, s, sr)
        lines.append(" ---> ".join(str(p) for p in paths))
        sigs.append((h, x, y))
    lst = tmp_path / "triples_list.txt"
    lst.write_text("\n".join(lines) + "\n")
    return lst, sigs


def test_eval_cli_estoi_column_and_unchanged_default(tmp_path, capsys):
    from flowdec_amd import eval_cli, metrics
    lst, sigs = make_triples(tmp_path, [0.9, 0.4, 0.7])
    base, with_estoi = tmp_path / "base.csv", tmp_path / "estoi.csv"
    r0 = eval_cli.run(["--triples", str(lst), "--out", str(base), "--sr", "16000", "--batch-files", "2"], scorer=eval_cli.HOST_SCORER)
    capsys.readouterr()
    r1 = eval_cli.run(["--triples", str(lst), "--out", str(with_estoi), "--sr", "16000", "--batch-files", "2", "--estoi"], scorer=eval_cli.HOST_SCORER)
    cap = capsys.readouterr()
    # without the flag: the pinned header, four columns, four means
    h0, rows0 = read_csv(base)
    assert tuple(h0) == eval_cli.CSV_HEADER and all(len(r) == 8 for r in rows0) and [m[0] for m in r0.means] == list(eval_cli.METRIC_NAMES)
    assert eval_cli.METRIC_NAMES == ("sisdr", "sisir", "sisar", "logspec_mse")
    # with it: one more column at the end, the others byte for byte
    h1, rows1 = read_csv(with_estoi)
    assert h1 == h0 + ["estoi"] and [r[:8] for r in rows1] == rows0
    assert [m[0] for m in r1.means] == list(eval_cli.METRIC_NAMES) + ["estoi"] and r1.means[:4] == r0.means
    # the wav files are 16-bit: score what was written
    from flowdec_amd.eval_cli import load_mono
    for i, r in enumerate(rows1):
        h, x = load_mono(r[1], 16000).numpy(), load_mono(r[2], 16000).numpy()
        assert float(r[8]) == metrics.estoi(h, x, 16000)
    assert rows1[1][8] == "1e-05" and "enh_1.wav" in cap.err and "fewer than 30 spectral frames" in cap.err
    assert float(rows1[0][8]) < float(rows1[2][8]) < 1.0                     # the estimates get cleaner along the list
    assert "estoi" in cap.out and cap.out.count("mean =") == 5
    with open(base, "rb") as f:
        four = f.read()
    assert four.splitlines()[0] == b",".join(s.encode() for s in eval_cli.CSV_HEADER)
    # score(): [n, 4] by default, [n, 5] with estoi; unequal lengths stay NaN in every column
    sig_t = [tuple(torch.from_numpy(a) for a in s) for s in sigs]
    assert eval_cli.score(sig_t, 16000, 2, eval_cli.HOST_SCORER).shape == (3, 4)
    bad = sig_t + [(sig_t[0][0][:-1], sig_t[0][1], sig_t[0][2])]
    v = eval_cli.score(bad, 16000, 2, eval_cli.HOST_SCORER, estoi=True)
    assert v.shape == (4, 5) and np.isnan(v[3]).all() and np.isfinite(v[:3]).all()
    # a Scorer without the third field still scores the four metrics
    assert eval_cli.Scorer(eval_cli.HOST_SCORER.si_sxr, eval_cli.HOST_SCORER.logspec).estoi is None


def test_enhance_cli_passes_estoi_through(monkeypatch):
    from flowdec_amd import enhance_cli, eval_cli
    base = ["--ckpt", "c", "--files", "f", "--outdir", "o", "--N", "3"]
    try:
        args = enhance_cli.build_parser().parse_args(base + ["--eval", "--eval-estoi"])
    except SystemExit:
        pytest.fail("enhance_cli refuses --eval --eval-estoi")
    assert args.eval and args.eval_estoi and not enhance_cli.build_parser().parse_args(base + ["--eval"]).eval_estoi
    seen = []
    monkeypatch.setattr(eval_cli, "run", lambda argv, **kw: seen.append(list(argv)))
    monkeypatch.setattr(torch.cuda, "device", lambda d: __import__("contextlib").nullcontext())
    args.device, args.batch_files = "cuda", 4
    enhance_cli.evaluate_triples(args, "")
    args.eval_estoi = False
    enhance_cli.evaluate_triples(args, "")
    assert seen[0][-1] == "--estoi" and "--estoi" not in seen[1] and seen[0][:-1] == seen[1]


def test_symbols_and_refusals_without_a_gpu():
    import __graft_entry__ as g
    g.build()
    from flowdec_amd import _lib
    lib = _lib.load()
    src = open(os.path.join(g.ROOT, "include", "flowdec_hip.h")).read()
    for name in ("fd_estoi_plan_create", "fd_estoi_plan_destroy", "fd_metrics_estoi_workspace_bytes", "fd_metrics_estoi_max_frames", "fd_metrics_estoi",
                 "fd_metrics_estoi_bands"):
        assert name + "(" in src and hasattr(lib, name) and name in _lib.SIGNATURES
    # sizes: host arithmetic only
    assert lib.fd_metrics_estoi_max_frames(48000, 24, 5) == 77 and lib.fd_metrics_estoi_max_frames(10000, 1, 1) == 77
    assert lib.fd_metrics_estoi_max_frames(256, 1, 1) == 1 and lib.fd_metrics_estoi_max_frames(385, 1, 1) == 2
    assert lib.fd_metrics_estoi_workspace_bytes(0, 48000, 24, 5) == 0 and lib.fd_metrics_estoi_workspace_bytes(2, 0, 24, 5) == 0
    assert lib.fd_metrics_estoi_workspace_bytes(2, 48000, 0, 5) == 0
    need = lib.fd_metrics_estoi_workspace_bytes(2, 48000, 24, 5)
    assert need > lib.fd_metrics_estoi_workspace_bytes(2, 10000, 1, 1) > 0 and need >= 2 * 2 * 10000 * 4
    # refusals are decided before any pointer is read and before anything is launched: dummy non-NULL pointers suffice
    buf = (C.c_char * 64)()
    p = C.cast(buf, C.c_void_p)
    err = lambda: lib.fd_last_error().decode()
    assert lib.fd_metrics_estoi(None, None, p, p, p, 2, 10000, p, p, p, 1 << 30, None) == FD_EINVAL and "fd_metrics_estoi: null pointer" in err()
    assert lib.fd_metrics_estoi(p, None, p, p, p, 2, 10000, None, p, p, 1 << 30, None) == FD_EINVAL and "null pointer" in err()
    assert lib.fd_metrics_estoi_bands(p, None, p, p, p, 2, 10000, p, None, p, p, 1 << 30, None) == FD_EINVAL and "fd_metrics_estoi_bands: null pointer" in err()
    assert lib.fd_metrics_estoi(p, None, p, p, p, 0, 10000, p, p, p, 1 << 30, None) == FD_EINVAL and "bad batch B 0" in err()
    small = lib.fd_metrics_estoi_workspace_bytes(2, 10000, 1, 1) - 1
    assert lib.fd_metrics_estoi(p, None, p, p, p, 2, 10000, p, p, p, small, None) == FD_EINVAL and "workspace too small" in err()
    assert lib.fd_estoi_plan_create(None) == FD_EINVAL and "null out" in err()
    lib.fd_estoi_plan_destroy(None)
