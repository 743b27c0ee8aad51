"""The spectral distances without a GPU: the host yardsticks of flowdec_amd.specdist (NumPy float64) against an independent restatement
with torch.stft, the mel filter bank's defining properties, the host tables of the GPU path (fd_specdist_tables), eval_cli --spectral with
the host scorer, and the refusals of the native entry points that are decided before anything is launched.

Parity of the bank with torchaudio.functional.melscale_fbanks is NOT pinned (torchaudio is not installed; scripts/pin_mel.py prints it
where it is)."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from test_eval_cpu import read_csv, write_wav

FD_EINVAL = -1
LENGTHS = (2049, 4095, 4096, 6000, 9001)
SR = 48000


def signals(n, seed):
    """x = 0.05 randn + 0.3 sin(2 pi 440 t) + 0.1 sin(2 pi 9000 t) at 48 kHz, x_hat = x + 0.02 randn; float32."""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / SR
    x = 0.05 * rng.standard_normal(n) + 0.3 * np.sin(2 * np.pi * 440 * t) + 0.1 * np.sin(2 * np.pi * 9000 * t)
    return (x + 0.02 * rng.standard_normal(n)).astype(np.float32), x.astype(np.float32)


def torch_spec(a, n_fft):
    return torch.stft(torch.from_numpy(np.asarray(a, np.float64)), n_fft, hop_length=n_fft // 4, win_length=n_fft,
                      window=torch.hann_window(n_fft, periodic=True, dtype=torch.float64), center=True, pad_mode="reflect", return_complex=True)


def torch_msstft(x_hat, x):
    loss = 0.0
    for n_fft in (4096, 2048, 1024, 512):
        A, R = torch_spec(x_hat, n_fft).abs(), torch_spec(x, n_fft).abs()
        loss += float((A.clamp(1e-5).pow(2).log10() - R.clamp(1e-5).pow(2).log10()).abs().mean())
        loss += float((A - R).abs().mean())
    return loss


def torch_mel(x_hat, x, sr):
    from flowdec_amd import specdist
    loss = 0.0
    for n_fft, n_mels in ((128, 10), (256, 20), (512, 40), (1024, 80), (2048, 160), (4096, 320)):
        fb = torch.from_numpy(specdist.mel_filterbank(sr, n_fft, n_mels))
        Mh = torch.matmul(torch_spec(x_hat, n_fft).abs().pow(2).transpose(0, 1), fb)
        Mx = torch.matmul(torch_spec(x, n_fft).abs().pow(2).transpose(0, 1), fb)
        loss += float((Mh.clamp(1e-5).pow(2).log10() - Mx.clamp(1e-5).pow(2).log10()).abs().mean())
    return loss


@pytest.mark.parametrize("n", LENGTHS)
def test_yardsticks_equal_torch_stft_float64(n):
    from flowdec_amd import specdist
    x_hat, x = signals(n, n)
    for n_fft in (128, 512, 4096):                               # torch.stft takes every length at every scale; T = 1 + L // hop
        S = torch_spec(x, n_fft)
        assert S.shape == (n_fft // 2 + 1, 1 + n // (n_fft // 4))
        assert np.allclose(specdist.stft(x, n_fft), S.numpy().T, rtol=0, atol=1e-12 * float(S.abs().max()))
    got, want = specdist.multiscale_stft_distance(x_hat, x), torch_msstft(x_hat, x)
    assert abs(got - want) <= 1e-12 * want, (got, want)
    got, want = specdist.mel_distance(x_hat, x, SR), torch_mel(x_hat, x, SR)
    assert abs(got - want) <= 1e-12 * want, (got, want)
    d = specdist.detail(x_hat, x, SR)
    assert d["msstft"] == specdist.multiscale_stft_distance(x_hat, x) or abs(d["msstft"] - specdist.multiscale_stft_distance(x_hat, x)) < 1e-14
    assert abs(d["mel"] - specdist.mel_distance(x_hat, x, SR)) < 1e-14 and len(d["scales"]) == 6


def test_yardstick_properties():
    from flowdec_amd import specdist
    x_hat, x = signals(6000, 1)
    assert specdist.multiscale_stft_distance(x, x) == 0.0 and specdist.mel_distance(x, x) == 0.0
    assert math.isnan(specdist.multiscale_stft_distance(x_hat[:2048], x[:2048])) and math.isnan(specdist.mel_distance(x_hat[:2048], x[:2048]))
    assert specdist.multiscale_stft_distance(x_hat[:2049], x[:2049]) > 0 and specdist.MIN_SAMPLES == 2049
    near, far = x + 0.25 * (x_hat - x), x_hat
    assert 0 < specdist.multiscale_stft_distance(near, x) < specdist.multiscale_stft_distance(far, x)
    assert 0 < specdist.mel_distance(near, x) < specdist.mel_distance(far, x)
    with pytest.raises(ValueError):
        specdist.mel_distance(x_hat[:-1], x)
    assert specdist.MSSTFT_SCALES == (4096, 2048, 1024, 512) and specdist.MEL_SCALES[0] == (128, 10) and specdist.MEL_SCALES[-1] == (4096, 320)


@pytest.mark.parametrize("sr,n_fft,n_mels", [(48000, 128, 10), (48000, 256, 20), (48000, 512, 40), (48000, 1024, 80), (48000, 2048, 160),
                                             (48000, 4096, 320), (16000, 512, 40)])
def test_mel_bank_properties(sr, n_fft, n_mels):
    from flowdec_amd import specdist
    fb = specdist.mel_filterbank(sr, n_fft, n_mels)
    F = n_fft // 2 + 1
    assert fb.shape == (F, n_mels) and fb.dtype == np.float64 and np.all(fb >= 0)
    assert np.all((fb > 0).sum(axis=0) >= 1)                     # no empty filter
    assert np.all((fb > 0).sum(axis=1) <= 2)                     # a bin lies under at most two triangles
    p = specdist.mel_points(sr, n_mels)
    assert p.shape == (n_mels + 2,) and p[0] == 0.0 and abs(p[-1] - sr // 2) <= 1e-9 * (sr // 2) and np.all(np.diff(p) > 0)
    mel = 2595.0 * np.log10(1.0 + p / 700.0)
    assert np.allclose(np.diff(mel), mel[-1] / (n_mels + 1), rtol=1e-12)                  # equally spaced on the HTK mel scale
    freqs = np.linspace(0, sr // 2, F)
    for j in range(n_mels):
        inside = (freqs > p[j]) & (freqs < p[j + 2])
        assert np.all(fb[~inside, j] == 0) and np.all(fb[inside, j] > 0)                  # zero outside (f_pts[j], f_pts[j+2])
        # the slaney factor: without it the triangle peaks at 1 in p[j+1]; its value at a bin is the linear interpolation
        tri = fb[:, j] / (2.0 / (p[j + 2] - p[j]))
        want = np.interp(freqs, [p[j], p[j + 1], p[j + 2]], [0.0, 1.0, 0.0], left=0.0, right=0.0)
        assert np.allclose(tri, want, rtol=0, atol=1e-12)


def test_mel_bank_hand_values():
    """(48 kHz, 128, 10): bins 375 Hz apart; edges from mel(24000) = 2595 log10(1 + 24000 / 700) = 4016.0191798718, steps of 4016.0191798718 / 11."""
    from flowdec_amd import specdist
    fb = specdist.mel_filterbank(48000, 128, 10)
    p = [700.0 * (10.0 ** (i * 4016.0191798718 / 11 / 2595.0) - 1.0) for i in range(12)]
    assert abs(p[1] - 267.8072035) < 1e-6 and abs(p[2] - 638.0725475) < 1e-6 and abs(p[9] - 12221.5714294) < 1e-6
    # bin 1 (375 Hz): falling side of filter 0 (0, 267.8, 638.1), rising side of filter 1 (267.8, 638.1, 1150.0)
    assert abs(fb[1, 0] - (p[2] - 375.0) / (p[2] - p[1]) * 2.0 / (p[2] - p[0])) < 1e-12 and abs(fb[1, 0] - 0.0022270112) < 1e-9
    assert abs(fb[1, 1] - (375.0 - p[1]) / (p[2] - p[1]) * 2.0 / (p[3] - p[1])) < 1e-12 and abs(fb[1, 1] - 0.0006563291) < 1e-9
    # bin 7 (2625 Hz): between the centres of filters 3 (1857.8) and 4 (2836.3)
    assert abs(fb[7, 3] - 0.0002561248) < 1e-9 and abs(fb[7, 4] - 0.0006725700) < 1e-9 and np.count_nonzero(fb[7]) == 2
    # bin 40 (15000 Hz): filters 8 and 9; the last bin (24000 Hz = the last edge) is under no filter
    assert abs(fb[40, 8] - 0.00010282) < 1e-9 and abs(fb[40, 9] - 0.0000954338) < 1e-9 and np.count_nonzero(fb[64]) == 0


@pytest.mark.parametrize("sr,n_fft,n_mels", [(48000, 128, 10), (48000, 256, 20), (48000, 512, 40), (48000, 1024, 80), (48000, 2048, 160),
                                             (48000, 4096, 320), (16000, 512, 40)])
def test_tables_equal_the_float64_formulas(sr, n_fft, n_mels):
    from flowdec_amd import specdist
    win, tw, first, count, w = specdist.tables(sr, n_fft, n_mels)
    k = np.arange(n_fft, dtype=np.float64)
    assert np.array_equal(win, (0.5 - 0.5 * np.cos(2 * np.pi * k / n_fft)).astype(np.float32))
    # the twiddles are the float32 rounding of the exact values: within half a float32 ulp of the float64 formula (whose own error, 1e-16,
    # is what separates cos(pi / 2) = 6e-17 in float64 from the table's exact 0), and equal to its plain rounding everywhere else
    m = np.arange(n_fft // 2, dtype=np.float64)
    want = np.stack([np.cos(2 * np.pi * m / n_fft), -np.sin(2 * np.pi * m / n_fft)], axis=1)
    assert tw.shape == want.shape and np.all(np.abs(tw - want) <= 2.0 ** -24 * np.abs(want) + 1e-16)
    differ = np.argwhere(tw != want.astype(np.float32))
    assert [tuple(d) for d in differ] in ([], [(n_fft // 4, 0)]) and tuple(tw[n_fft // 4]) == (0.0, -1.0) and tuple(tw[0]) == (1.0, 0.0)
    # W^(N/2 - m) = (-re, im) of W^m, bit for bit: what makes x_hat == x score exactly 0 on the GPU
    assert np.array_equal(tw[1:][::-1, 0], -tw[1:, 0]) and np.array_equal(tw[1:][::-1, 1], tw[1:, 1])
    # the banded bank expands to mel_filterbank rounded to float32
    fb = specdist.mel_filterbank(sr, n_fft, n_mels).astype(np.float32)
    assert first.shape == count.shape == (n_mels,) and len(w) == int(count.sum()) and np.all(count >= 1) and np.all(first + count <= n_fft // 2 + 1)
    expanded, o = np.zeros_like(fb), 0
    for j in range(n_mels):
        expanded[first[j]:first[j] + count[j], j] = w[o:o + count[j]]
        o += count[j]
    assert np.array_equal(expanded, fb) and np.all(w > 0)


def test_symbols_and_refusals_without_a_gpu():
    import os
    import __graft_entry__ as g
    g.build()
    from flowdec_amd import _lib, specdist
    lib = _lib.load()
    src = open(os.path.join(g.ROOT, "include", "flowdec_hip.h")).read()
    names = ("fd_specdist_tables", "fd_specdist_plan_create", "fd_specdist_plan_destroy", "fd_metrics_specdist_workspace_bytes", "fd_metrics_specdist",
             "fd_metrics_specdist_spectra")
    for name in names:
        assert name + "(" in src and hasattr(lib, name) and name in _lib.SIGNATURES
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
    err = lambda: lib.fd_last_error().decode()
    buf = (C.c_char * 64)()
    p = C.cast(buf, C.c_void_p)
    # the tables: window lengths are powers of two in [128, 4096]
    for bad in (1000, 64, 8192, 0, -128):
        assert lib.fd_specdist_tables(48000, bad, 0, None, None, None, None, None) == FD_EINVAL and "power of two in [128, 4096]" in err()
    assert lib.fd_specdist_tables(48000, 128, 65, None, None, None, None, None) == FD_EINVAL and "n_mels" in err()
    assert lib.fd_specdist_tables(48000, 128, 10, None, None, None, None, None) == int(specdist.tables(48000, 128, 10)[3].sum())
    assert lib.fd_specdist_tables(48000, 128, 0, None, None, None, None, None) == 0
    assert lib.fd_specdist_tables(48000, 128, 10, p, None, p, p, p) == FD_EINVAL and "fd_specdist_tables: null pointer" in err()
    assert lib.fd_specdist_tables(48000, 128, 10, p, p, p, p, None) == FD_EINVAL and "null pointer" in err()
    assert lib.fd_specdist_tables(48000, 128, 64, None, None, None, None, None) == FD_EINVAL and "empty" in err()       # 64 filters over 65 bins
    # the plan: every refusal comes before the first device call
    ints = lambda *v: (C.c_int * len(v))(*v)
    h = C.c_void_p()
    assert lib.fd_specdist_plan_create(48000, 1, ints(512), ints(40), ints(1), None) == FD_EINVAL and "null out" in err()
    assert lib.fd_specdist_plan_create(48000, 1, None, ints(40), ints(1), C.byref(h)) == FD_EINVAL and "null pointer" in err()
    for bad in (1000, 64, 8192):
        assert lib.fd_specdist_plan_create(48000, 2, ints(512, bad), ints(40, 0), ints(1, 1), C.byref(h)) == FD_EINVAL and "power of two" in err()
        assert not h.value
    assert lib.fd_specdist_plan_create(48000, 0, ints(512), ints(40), ints(1), C.byref(h)) == FD_EINVAL and "n_scales" in err()
    assert lib.fd_specdist_plan_create(48000, 17, ints(*[512] * 17), ints(*[0] * 17), ints(*[1] * 17), C.byref(h)) == FD_EINVAL and "n_scales" in err()
    assert lib.fd_specdist_plan_create(48000, 1, ints(512), ints(0), ints(0), C.byref(h)) == FD_EINVAL and "neither" in err()
    assert lib.fd_specdist_plan_create(48000, 1, ints(512), ints(257), ints(0), C.byref(h)) == FD_EINVAL and "n_mels" in err()
    lib.fd_specdist_plan_destroy(None)
    # the calls: a NULL plan or pointer is refused before anything is read; so is a workspace query with a bad plan or batch
    assert lib.fd_metrics_specdist_workspace_bytes(None, 2, 9001) == 0 and lib.fd_metrics_specdist_workspace_bytes(None, 0, 9001) == 0
    assert lib.fd_metrics_specdist(None, p, p, p, 2, 9001, p, None, p, 1 << 30, None) == FD_EINVAL and "fd_metrics_specdist: null pointer" in err()
    assert lib.fd_metrics_specdist_spectra(None, 0, p, p, p, 2, 9001, p, p, None, None, p, 1 << 30, None) == FD_EINVAL \
        and "fd_metrics_specdist_spectra: null pointer" in err()


def make_triples(tmp_path, lengths, seed=0):
    lines = []
    for i, n in enumerate(lengths):
        h, x = signals(n, seed + i)
        y = (x + 0.1 * np.random.default_rng(100 + i).standard_normal(n)).astype(np.float32)
        paths = [tmp_path / f"clean_{i}.wav", tmp_path / f"noisy_{i}.wav", tmp_path / f"enh_{i}.wav"]
        for path, s in zip(paths, (x, y, h)):
            write_wav(path, s, SR)
        lines.append(" ---> ".join(str(q) for q in paths))
    lst = tmp_path / "triples_list.txt"
    lst.write_text("\n".join(lines) + "\n")
    return lst


def test_eval_cli_spectral_columns_and_unchanged_default(tmp_path, capsys):
    from flowdec_amd import eval_cli, specdist
    from flowdec_amd.eval_cli import load_mono
    lst = make_triples(tmp_path, [4800, 2048, 9600])             # 0.1 s, one sample under the 2049-sample rule, 0.2 s
    out = {k: tmp_path / f"{k}.csv" for k in ("base", "estoi", "spectral", "both")}
    flags = dict(base=[], estoi=["--estoi"], spectral=["--spectral"], both=["--estoi", "--spectral"])
    res, caps = {}, {}
    for k in out:
        res[k] = eval_cli.run(["--triples", str(lst), "--out", str(out[k]), "--batch-files", "2"] + flags[k], scorer=eval_cli.HOST_SCORER)
        caps[k] = capsys.readouterr()
    heads, rows = {}, {}
    for k in out:
        heads[k], rows[k] = read_csv(out[k])
    # without --spectral: the pinned headers; the bytes are those of the writer without the columns= argument on the same values
    assert tuple(heads["base"]) == eval_cli.CSV_HEADER and tuple(heads["estoi"]) == eval_cli.CSV_HEADER + ("estoi",)
    triples = eval_cli.read_triples(str(lst))
    for k, ncol in (("base", 4), ("estoi", 5)):
        vals = np.array([[float(v) for v in r[4:]] for r in rows[k]])
        assert vals.shape == (3, ncol)
        eval_cli.write_csv(str(tmp_path / "again.csv"), triples, vals)
        assert (tmp_path / "again.csv").read_bytes() == out[k].read_bytes()
        assert eval_cli.summary(vals) == res[k].means and len(res[k].means) == ncol
        assert "msstft" not in caps[k].out and "2049" not in caps[k].err
    # with it: two last columns, the others byte for byte
    assert heads["spectral"] == heads["base"] + ["msstft", "mel"] and heads["both"] == heads["estoi"] + ["msstft", "mel"]
    assert [r[:8] for r in rows["spectral"]] == rows["base"] and [r[:9] for r in rows["both"]] == rows["estoi"]
    assert [r[-2:] for r in rows["both"]] == [r[-2:] for r in rows["spectral"]]
    assert [m[0] for m in res["spectral"].means] == list(eval_cli.METRIC_NAMES) + ["msstft", "mel"] and res["spectral"].means[:4] == res["base"].means
    assert [m[0] for m in res["both"].means] == list(eval_cli.METRIC_NAMES) + ["estoi", "msstft", "mel"]
    assert caps["spectral"].out.count("mean =") == 6 and caps["both"].out.count("mean =") == 7 and "msstft" in caps["spectral"].out
    # the 2048-sample triple: NaN in exactly those two columns, and a warning naming the rule
    short = rows["both"][1]
    assert short[-2:] == ["nan", "nan"] and all(v != "nan" for v in short[4:8]) and "enh_1.wav" in caps["both"].err and "2049" in caps["both"].err
    assert res["spectral"].means[-1][2] == 2 and res["spectral"].means[-2][2] == 2
    # the wav files are 16-bit: score what was written
    for i in (0, 2):
        r = rows["spectral"][i]
        h, x = load_mono(r[1], SR).numpy(), load_mono(r[2], SR).numpy()
        assert float(r[-2]) == specdist.multiscale_stft_distance(h, x) and float(r[-1]) == specdist.mel_distance(h, x, SR)
        assert 0 < float(r[-2]) and 0 < float(r[-1])
    # score(): the column layout; unequal lengths stay NaN everywhere; a Scorer without the field refuses
    assert eval_cli.metric_columns(True, True) == eval_cli.METRIC_NAMES + ("estoi", "msstft", "mel")
    sig = [tuple(torch.from_numpy(a) for a in (signals(4800, 5) + (signals(4800, 6)[1],)))]
    bad = sig + [(sig[0][0][:-1], sig[0][1], sig[0][2])]
    v = eval_cli.score(bad, SR, 2, eval_cli.HOST_SCORER, spectral=True)
    assert v.shape == (2, 6) and np.isnan(v[1]).all() and np.isfinite(v[0]).all()
    with pytest.raises(ValueError):
        eval_cli.score(sig, SR, 2, eval_cli.Scorer(eval_cli.HOST_SCORER.si_sxr, eval_cli.HOST_SCORER.logspec), spectral=True)
    with pytest.raises(ValueError):
        eval_cli.write_csv(str(tmp_path / "x.csv"), triples[:1], v[:1], columns=eval_cli.METRIC_NAMES)
    assert eval_cli.GPU_SCORER.spectral is not None and eval_cli.HOST_SCORER.spectral is not None


def test_parser_flags_of_both_command_lines(monkeypatch):
    from flowdec_amd import enhance_cli, eval_cli
    a = eval_cli.build_parser().parse_args(["--triples", "t", "--out", "o"])
    assert not a.spectral and not a.estoi
    a = eval_cli.build_parser().parse_args(["--triples", "t", "--out", "o", "--spectral", "--estoi"])
    assert a.spectral and a.estoi
    base = ["--ckpt", "c", "--files", "f", "--outdir", "o", "--N", "3"]
    args = enhance_cli.build_parser().parse_args(base + ["--eval", "--eval-spectral"])
    assert args.eval and args.eval_spectral and not args.eval_estoi and not enhance_cli.build_parser().parse_args(base + ["--eval"]).eval_spectral
    seen = []
    monkeypatch.setattr(eval_cli, "run", lambda argv, **kw: seen.append(list(argv)))
    monkeypatch.setattr(torch.cuda, "device", lambda d: __import__("contextlib").nullcontext())
    args.device, args.batch_files = "cuda", 4
    enhance_cli.evaluate_triples(args, "")
    args.eval_estoi = True
    enhance_cli.evaluate_triples(args, "")
    args.eval_spectral = False
    enhance_cli.evaluate_triples(args, "")
    assert seen[0][-1] == "--spectral" and seen[1][-2:] == ["--estoi", "--spectral"] and seen[2][-1] == "--estoi" and seen[0][:-1] == seen[2][:-1]
