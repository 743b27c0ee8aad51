"""The segmental SNRs without a GPU: the host yardsticks of flowdec_amd.segsnr (NumPy float64) against a direct transcription of the
published algorithm that goes through scipy.signal.stft, the frame rule, the critical-band bank's defining properties, hand values, the
host tables of the GPU path (fd_segsnr_tables), the refusals of the native entry points that are decided before anything is launched,
eval_cli --ssnr with the host scorer, and -- in float32 NumPy -- why the packed transform of csrc/segsnr.hip scales every frame first.

Parity with the pysepm package is NOT pinned (pysepm is not installed; scripts/pin_segsnr.py prints it where it is).

The bank: the bandwidths are the table of comp_fwseg.m, band_i = cent_(i+1) - cent_i (seven bands of 70 Hz; checked below).  With it the
widest filter (346.136 Hz at 3597.63 Hz) has f0 = 306 and bw = 29.54 bins at 48 kHz; its taps above exp(-30 / 4.606) satisfy
11 q^2 < 6.5132 - ln(346.136 / 70), |j - f0| < 19.74: 39 taps, the last one at bin 325.  (A table that repeats 70 Hz once more and stops at
321.465 Hz would give 37 taps and bin 324; that is not the published one.)"""
import ctypes as C
import math

import numpy as np
import pytest
import scipy.signal
import torch

from test_eval_cpu import read_csv, write_wav

FD_EINVAL = -1
RATES = (8000, 16000, 48000)
DIMS = {8000: (240, 60, 512), 16000: (480, 120, 1024), 48000: (1440, 360, 4096)}
EPS = 2.0 ** -52


def clean(n, sr, seed):
    """x = 0.05 randn + 0.3 sin(2 pi 440 t) + 0.1 sin(2 pi 1800 t), float64."""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / sr
    return 0.05 * rng.standard_normal(n) + 0.3 * np.sin(2 * np.pi * 440 * t) + 0.1 * np.sin(2 * np.pi * 1800 * t)


def pair(n, sr, seed, kind):
    """(x_hat, x) float32.  kind: a number = white noise at that SNR in dB; 'gap' = 20 dB and a zeroed stretch inside x (and x_hat); 'tail' =
    20 dB and the last four windows of x_hat zeroed; 'head' = 20 dB and the first four windows of x_hat times 1e-6; 'tail+head' = both."""
    rng = np.random.default_rng(1000 + seed)
    x = clean(n, sr, seed)
    snr = kind if isinstance(kind, (int, float)) else 20.0
    noise = rng.standard_normal(n)
    h = x + noise * np.sqrt(np.mean(x ** 2) / np.mean(noise ** 2)) * 10.0 ** (-snr / 20.0)
    win = DIMS[sr][0] if sr in DIMS else round(0.03 * sr)
    if kind == "gap":
        x[n // 3:n // 3 + 3 * win] = 0.0
        h[n // 3:n // 3 + 3 * win] = 0.0
    if isinstance(kind, str) and "tail" in kind:
        h[n - 4 * win:] = 0.0
    if isinstance(kind, str) and "head" in kind:
        h[:4 * win] *= 1e-6
    return h.astype(np.float32), x.astype(np.float32)


# (sr, samples, kind): at 8 kHz (N 512, two frames per workgroup) T = 1, 6, 7, 62, 289 and one clip under win + skip = 300; at 16 kHz
# (N 1024, one frame per workgroup) T = 1, 4, 62; one 48 kHz clip (N 4096), T = 29.  Every clip but the 2.2 s one is 0.5 s or shorter.
CASES = ((8000, 300, 40), (8000, 617, 30), (8000, 673, 20), (8000, 299, 10), (8000, 4000, 0), (8000, 3971, -15), (8000, 4000, "gap"),
         (8000, 4000, "tail"), (8000, 4000, "head"), (8000, 17600, 10),
         (16000, 600, 30), (16000, 1000, -15), (16000, 8000, "tail"), (16000, 7993, "head"), (16000, 8000, 0),
         (48000, 12007, "tail+head"))


def case_pairs(sr):
    """The case set of one rate -> [(x_hat, x)] and the cases, in CASES order."""
    cases = [c for c in CASES if c[0] == sr]
    return [pair(n, sr, 10 * i + sr // 8000, kind) for i, (_, n, kind) in enumerate(cases)], cases


def transcription(x_hat, x, sr):
    """fwSNRseg and SNRseg as published, written out again through scipy.signal.stft and a frame loop -> (fwSSNR, frames, SSNR, frames)."""
    eps = np.finfo(np.float64).eps
    clean_speech, processed_speech = np.asarray(x, np.float64), np.asarray(x_hat, np.float64)
    winlength = round(0.03 * sr)
    skiprate = int(np.floor((1 - 0.75) * 0.03 * sr))
    n_fft = 2 ** int(np.ceil(np.log2(2 * winlength)))
    hann = 0.5 * (1 - np.cos(2 * np.pi * np.arange(1, winlength + 1) / (winlength + 1)))
    # SNRseg: every full frame, the last one removed
    count = (len(clean_speech) - winlength + skiprate) // skiprate
    seg = []
    for t in range(count):
        a = hann * clean_speech[t * skiprate:t * skiprate + winlength]
        b = hann * processed_speech[t * skiprate:t * skiprate + winlength]
        seg.append(10 * np.log10(np.sum(a ** 2) / (np.sum((a - b) ** 2) + eps) + eps))
    seg = np.clip(np.array(seg[:-1]), -10, 35)
    # fwSNRseg
    from flowdec_amd import segsnr
    bank = segsnr.critical_band_bank(sr, n_fft)
    num_frames = int(len(clean_speech) / skiprate - (winlength / skiprate))
    cut = num_frames * skiprate + winlength - skiprate

    def spec(sig):
        _, _, Z = scipy.signal.stft((sig + eps)[:cut], fs=sr, window=hann, nperseg=winlength, noverlap=winlength - skiprate, nfft=n_fft, detrend=False,
                                    return_onesided=True, boundary=None, padded=False)
        S = np.abs(Z)[:-1, :]
        return S / S.sum(0)
    ce, pe = bank.dot(spec(clean_speech)), bank.dot(spec(processed_speech))
    err = np.power(ce - pe, 2)
    err[err < eps] = eps
    wf = np.power(ce, 0.2)
    fw = np.clip(np.sum(wf * (10 * np.log10(ce ** 2 / err)), 0) / np.sum(wf, 0), -10, 35)
    return float(np.mean(fw)), fw.shape[0], float(np.mean(seg)), len(seg)


@pytest.mark.parametrize("sr", RATES)
def test_yardstick_equals_the_scipy_transcription(sr):
    from flowdec_amd import segsnr
    assert segsnr.frame_params(sr) == DIMS[sr]
    for i, (n, kind) in enumerate(((int(0.31 * sr) + 17, 15), (int(0.2 * sr), "tail"), (int(0.25 * sr) + 3, "gap"))):
        h, x = pair(n, sr, 50 + i, kind)
        d = segsnr.segsnr_detail(h, x, sr)
        fw, t_fw, ss, t_ss = transcription(h, x, sr)
        assert d["frames"] == t_fw == t_ss == (n - DIMS[sr][0]) // DIMS[sr][1]
        assert abs(d["fwssnr"] - fw) <= 1e-10 and abs(d["ssnr"] - ss) <= 1e-10, (d["fwssnr"] - fw, d["ssnr"] - ss)
        assert d["fwssnr"] == segsnr.fw_segmental_snr(h, x, sr) and d["ssnr"] == segsnr.segmental_snr(h, x, sr)
        assert d["fw_frames"].shape == d["ss_frames"].shape == (t_fw,) and -10 <= d["fw_frames"].min() and d["fw_frames"].max() <= 35


@pytest.mark.parametrize("sr", RATES)
def test_frame_rule(sr):
    from flowdec_amd import segsnr
    win, skip, _ = DIMS[sr]
    for n in (win + skip, win + skip + 1, win + 2 * skip - 1, win + 2 * skip, win + 7 * skip + skip // 2):
        T = (n - win) // skip
        assert segsnr.num_frames(n, sr) == T >= 1
        assert (n - win + skip) // skip - 1 == T                                          # SNRseg: all full frames but the last
        cut = int(n / skip - win / skip) * skip + win - skip                              # fwSNRseg: the cut, then an unpadded STFT
        assert (cut - win) // skip + 1 == T
        h, x = pair(n, sr, n % 97, 20)
        d = segsnr.segsnr_detail(h, x, sr)
        assert d["frames"] == T and len(d["fw_frames"]) == T and math.isfinite(d["fwssnr"]) and math.isfinite(d["ssnr"])
    h, x = pair(win + skip - 1, sr, 3, 20)
    assert segsnr.num_frames(win + skip - 1, sr) == 0 and segsnr.min_samples(sr) == win + skip
    assert math.isnan(segsnr.fw_segmental_snr(h, x, sr)) and math.isnan(segsnr.segmental_snr(h, x, sr))
    assert segsnr.segsnr_detail(h[:win - 5], x[:win - 5], sr)["frames"] == 0               # shorter than one window
    assert segsnr.segsnr_detail(*pair(win + skip, sr, 4, 20), sr)["frames"] == 1
    with pytest.raises(ValueError):
        segsnr.segmental_snr(h[:-1], x, sr)


@pytest.mark.parametrize("sr", RATES)
def test_bank_properties(sr):
    from flowdec_amd import segsnr
    _, _, n_fft = DIMS[sr]
    bank = segsnr.critical_band_bank(sr, n_fft)
    assert bank.shape == (25, n_fft // 2) and bank.dtype == np.float64 and segsnr.NUM_BANDS == 25
    f0 = segsnr.band_centres(sr, n_fft)
    floor = math.exp(-30.0 / (2 * 2.303))
    for i in range(25):
        nz = np.flatnonzero(bank[i])
        assert int(np.argmax(bank[i])) == f0[i] and abs(bank[i, f0[i]] - 70.0 / segsnr.BANDWIDTH[i]) <= 1e-15 * 70.0 / segsnr.BANDWIDTH[i]
        assert np.array_equal(nz, np.arange(nz[0], nz[-1] + 1)) and f0[i] - nz[0] == nz[-1] - f0[i]        # one run, symmetric about the peak
        assert np.all(bank[i, nz] > floor)
        left, right = bank[i, nz[0]:f0[i] + 1], bank[i, f0[i]:nz[-1] + 1]
        assert np.allclose(left, right[::-1], rtol=1e-14, atol=0)
    # the table itself: band_i = cent_(i+1) - cent_i to the table's own digits, seven bands of 70 Hz, the bands stop under 3.8 kHz
    cent, band = np.array(segsnr.CENT_FREQ), np.array(segsnr.BANDWIDTH)
    assert np.all(np.abs(np.diff(cent) - band[:-1]) < 0.0075) and list(band[:7]) == [70.0] * 7 and band[7] == 77.3724 and band[-1] == 346.136
    assert cent[-1] + band[-1] / 2 < 3800
    if sr == 48000:
        counts = (bank != 0).sum(axis=1)
        assert counts.max() == 39 and np.flatnonzero(bank.any(axis=0))[-1] == 325 and f0[-1] == 306         # (the module docstring derives both)
        assert np.all(bank[:, 326:] == 0)


@pytest.mark.parametrize("sr", RATES + (44100, 22050))
def test_tables_equal_the_float64_formulas(sr):
    from flowdec_amd import segsnr, specdist
    (win, skip, n_fft), w, tw, first, count, wgt = segsnr.tables(sr)
    assert (win, skip, n_fft) == segsnr.frame_params(sr)
    n = np.arange(win, dtype=np.float64)
    assert w.dtype == np.float64 and np.array_equal(w, segsnr.window(win))
    assert np.allclose(w, 0.5 * (1 - np.cos(2 * np.pi * (n + 1) / (win + 1))), rtol=0, atol=2e-16)          # NumPy's own cos: to the last bit or so
    assert np.array_equal(tw, specdist.tables(48000, n_fft, 0)[1])                                          # the shared transform's twiddles
    bank = segsnr.critical_band_bank(sr, n_fft)
    assert first.shape == count.shape == (25,) and len(wgt) == int(count.sum()) and np.all(count >= 1) and np.all(first + count <= n_fft // 2)
    expanded, o = np.zeros_like(bank), 0
    for i in range(25):
        expanded[i, first[i]:first[i] + count[i]] = wgt[o:o + count[i]]
        o += count[i]
    assert np.array_equal(expanded, bank) and np.all(wgt > 0)                                              # exactly: the same float64 operations


def test_hand_values():
    from flowdec_amd import segsnr
    sr, (win, skip, _) = 8000, DIMS[8000]
    n = win + 9 * skip + 5
    _, x = pair(n, sr, 7, 20)
    d = segsnr.segsnr_detail(x, x, sr)
    assert d["fwssnr"] == 35.0 and d["ssnr"] == 35.0 and np.all(d["fw_frames"] == 35.0)                     # x_hat = x, no silence
    d0 = segsnr.segsnr_detail(np.zeros_like(x), x, sr)
    assert np.all(np.abs(d0["ss_frames"]) < 1e-12) and abs(d0["ssnr"]) < 1e-12                               # x_hat = 0: 0 dB in every frame
    xs = x.copy()
    xs[:win + skip] = 0.0                                                                                    # frames 0 and 1 of x are digitally silent
    ds = segsnr.segsnr_detail(xs, xs, sr)
    assert ds["ss_frames"][0] == -10.0 and ds["ss_frames"][1] == -10.0 and np.all(ds["ss_frames"][5:] == 35.0)   # -10, not 35: the package's behaviour
    assert ds["ssnr"] == pytest.approx(np.mean(ds["ss_frames"]), abs=1e-12) and ds["ssnr"] < 35.0
    # one frame by hand: SSNR = 10 log10(sum (w x)^2 / sum (w (x - x_hat))^2), the eps terms far below
    h, x1 = pair(win + skip, sr, 8, 10)
    w = 0.5 * (1 - np.cos(2 * np.pi * np.arange(1, win + 1) / (win + 1)))
    a, b = w * x1[:win].astype(np.float64), w * h[:win].astype(np.float64)
    assert segsnr.segmental_snr(h, x1, sr) == pytest.approx(10 * np.log10(np.sum(a * a) / np.sum((a - b) ** 2)), abs=1e-9)
    # noisier is worse, in both
    near, far = pair(4000, sr, 9, 20), pair(4000, sr, 9, 0)
    assert segsnr.segmental_snr(*near, sr) > segsnr.segmental_snr(*far, sr) and segsnr.fw_segmental_snr(*near, sr) > segsnr.fw_segmental_snr(*far, sr)
    assert segsnr.NAMES == ("fwSSNR", "SSNR")


def packed_float32(x_hat, x, sr, scale):
    """fwSSNR per frame as csrc/segsnr.hip forms it, in NumPy: the frames of both signals as ONE complex64 sequence z = b' + i a' through a
    float32 FFT, unpacked, the rest in float64.  scale=True: each frame of each signal times the power of two that brings its peak into
    [1, 2) before the rounding to float32."""
    from flowdec_amd import segsnr
    win, skip, n_fft = segsnr.frame_params(sr)
    T, w, h = segsnr.num_frames(len(x), sr), segsnr.window(win), n_fft // 2
    view = lambda s: np.lib.stride_tricks.sliding_window_view(np.asarray(s, np.float64) + EPS, win)[::skip][:T] * w
    a, b = view(x), view(x_hat)
    if scale:
        a = a * 2.0 ** -np.floor(np.log2(np.abs(a).max(axis=1, keepdims=True)))
        b = b * 2.0 ** -np.floor(np.log2(np.abs(b).max(axis=1, keepdims=True)))
    z = np.zeros((T, n_fft), np.complex64)
    z[:, :win] = b.astype(np.float32) + 1j * a.astype(np.float32)
    Z = np.fft.fft(z, axis=1)
    assert Z.dtype == np.complex64
    Zn = np.conj(np.roll(Z[:, ::-1], 1, axis=1))                                           # conj Z_{N-k}
    P, Q = (0.5 * (Z + Zn))[:, :h], (-0.5j * (Z - Zn))[:, :h]
    proc, cl = np.abs(P.astype(np.complex128)), np.abs(Q.astype(np.complex128))
    proc, cl = proc / proc.sum(axis=1, keepdims=True), cl / cl.sum(axis=1, keepdims=True)
    bank = segsnr.critical_band_bank(sr, n_fft)
    ce, pe = cl @ bank.T, proc @ bank.T
    wf = ce ** 0.2
    return np.clip(np.sum(wf * 10 * np.log10(ce ** 2 / np.maximum((ce - pe) ** 2, EPS)), axis=1) / np.sum(wf, axis=1), -10, 35)


@pytest.mark.parametrize("sr", (8000, 48000))
def test_packed_float32_transform_needs_the_frame_scaling(sr):
    """A silent (eps w) or very quiet frame of one signal beside a normal frame of the other: packed into one float32 transform as they
    are, its spectrum is the other signal's rounding noise, and the measure, which divides every spectrum by its own sum, shows it in
    full.  Scaled first, the same transform stays within the 1e-3 dB that the CSV's digits ask of a clip."""
    from flowdec_amd import segsnr
    h, x = pair(int(0.25 * sr) + 7, sr, 21, "tail+head")
    d = segsnr.segsnr_detail(h, x, sr)
    plain, scaled = packed_float32(h, x, sr, False), packed_float32(h, x, sr, True)
    e_plain, e_scaled = abs(np.mean(plain) - d["fwssnr"]), abs(np.mean(scaled) - d["fwssnr"])
    print(f"packed float32 transform at {sr} Hz: clip error {e_plain:.3g} dB unscaled (worst frame {np.abs(plain - d['fw_frames']).max():.3g}), "
          f"{e_scaled:.3g} dB scaled (worst frame {np.abs(scaled - d['fw_frames']).max():.3g})")
    assert e_plain > 0.1 and np.abs(plain - d["fw_frames"]).max() > 1.0
    assert e_scaled < 1e-3 and np.abs(scaled - d["fw_frames"]).max() < 2e-2
    _, x2 = pair(4000, 8000, 22, 20)
    assert np.all(packed_float32(x2, x2, 8000, True) == 35.0)


def test_symbols_and_refusals_without_a_gpu():
    import os
    import __graft_entry__ as g
    g.build()
    from flowdec_amd import _lib, build, segsnr
    lib = _lib.load()
    src = open(os.path.join(g.ROOT, "include", "flowdec_hip.h")).read()
    names = ("fd_segsnr_tables", "fd_segsnr_plan_create", "fd_segsnr_plan_destroy", "fd_metrics_segsnr_workspace_bytes", "fd_metrics_segsnr")
    for name in names:
        assert name + "(" in src and hasattr(lib, name) and name in _lib.SIGNATURES
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
    assert "segsnr.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "fft_lds.h"))
    # the shared transform lives in the header alone
    spec_src, seg_src = (open(os.path.join(build.CSRC, f)).read() for f in ("specdist.hip", "segsnr.hip"))
    for text in (spec_src, seg_src):
        assert '#include "fft_lds.h"' in text and "fft_lds::passes<LOG2N>" in text and "__device__ __forceinline__ float2 cmul" not in text
    err = lambda: lib.fd_last_error().decode()
    buf = (C.c_char * 64)()
    p = C.cast(buf, C.c_void_p)
    # the tables: n_fft = 2^ceil(log2(2 round(0.03 sr))) in [128, 4096]; a rate under 7.2 kHz leaves the upper bands without a bin
    for bad in (0, -8000, 1000, 96000, 1 << 25):
        assert lib.fd_segsnr_tables(bad, None, None, None, None, None, None) == FD_EINVAL and "outside [128, 4096]" in err()
    assert lib.fd_segsnr_tables(4000, None, None, None, None, None, None) == FD_EINVAL and "empty" in err()
    dims = (C.c_int * 3)()
    assert lib.fd_segsnr_tables(48000, dims, None, None, None, None, None) == len(segsnr.tables(48000)[5]) and tuple(dims) == (1440, 360, 4096)
    assert lib.fd_segsnr_tables(48000, None, p, None, p, p, p) == FD_EINVAL and "fd_segsnr_tables: null pointer" in err()
    assert lib.fd_segsnr_tables(48000, None, p, p, p, p, None) == FD_EINVAL and "null pointer" in err()
    # the plan: every refusal comes before the first device call
    h = C.c_void_p()
    assert lib.fd_segsnr_plan_create(48000, None) == FD_EINVAL and "null out" in err()
    for bad in (1000, 96000):
        assert lib.fd_segsnr_plan_create(bad, C.byref(h)) == FD_EINVAL and "outside [128, 4096]" in err() and not h.value
    lib.fd_segsnr_plan_destroy(None)
    # the calls: a NULL plan or pointer is refused before anything is read; so is a workspace query with a bad plan
    assert lib.fd_metrics_segsnr_workspace_bytes(None, 2, 9001) == 0
    assert lib.fd_metrics_segsnr(None, p, p, p, 2, 9001, p, None, p, 1 << 30, None) == FD_EINVAL and "fd_metrics_segsnr: null pointer" in err()


SR = 48000


def make_triples(tmp_path, lengths, sr=SR, seed=0):
    lines = []
    for i, n in enumerate(lengths):
        h, x = pair(n, sr, seed + i, 15)
        y = (x + 0.1 * np.random.default_rng(100 + i).standard_normal(n)).astype(np.float32)
        paths = [tmp_path / f"clean_{i}.wav", tmp_path / f"noisy_{i}.wav", tmp_path / f"enh_{i}.wav"]
        for path, s in zip(paths, (x, y, h)):
            write_wav(path, s, sr)
        lines.append(" ---> ".join(str(q) for q in paths))
    lst = tmp_path / "triples_list.txt"
    lst.write_text("\n".join(lines) + "\n")
    return lst


def test_eval_cli_ssnr_columns_and_unchanged_default(tmp_path, capsys):
    from flowdec_amd import eval_cli, segsnr
    from flowdec_amd.eval_cli import load_mono
    lst = make_triples(tmp_path, [4800, 1799, 9600])             # 0.1 s, one sample under win + skip = 1800, 0.2 s
    flags = dict(base=[], ssnr=["--ssnr"], estoi=["--estoi"], estoi_ssnr=["--estoi", "--ssnr"], spectral=["--spectral"],
                 all=["--ssnr", "--estoi", "--spectral", "--loudness", "--align", "2", "--align-polarity"],
                 all_off=["--estoi", "--spectral", "--loudness", "--align", "2", "--align-polarity"], spectral_ssnr=["--spectral", "--ssnr"])
    out = {k: tmp_path / f"{k}.csv" for k in flags}
    res, caps, heads, rows = {}, {}, {}, {}
    for k in out:
        res[k] = eval_cli.run(["--triples", str(lst), "--out", str(out[k]), "--batch-files", "2"] + flags[k], scorer=eval_cli.HOST_SCORER)
        caps[k] = capsys.readouterr()
        heads[k], rows[k] = read_csv(out[k])
    # without --ssnr: the pinned header, and the bytes of the writer without the columns= argument on the same values
    assert tuple(heads["base"]) == eval_cli.CSV_HEADER and "SSNR" not in caps["base"].out and "win + skip" not in caps["base"].err
    triples = eval_cli.read_triples(str(lst))
    vals = np.array([[float(v) for v in r[4:]] for r in rows["base"]])
    eval_cli.write_csv(str(tmp_path / "again.csv"), triples, vals)
    assert (tmp_path / "again.csv").read_bytes() == out["base"].read_bytes() and eval_cli.summary(vals) == res["base"].means
    # with it: two columns behind every other metric and before lufs_* / lag_* / pol_*, the others byte for byte
    assert heads["ssnr"] == heads["base"] + ["fwSSNR", "SSNR"] and [r[:8] for r in rows["ssnr"]] == rows["base"]
    assert heads["estoi_ssnr"] == heads["estoi"] + ["fwSSNR", "SSNR"] and [r[:9] for r in rows["estoi_ssnr"]] == rows["estoi"]
    assert heads["spectral_ssnr"] == heads["spectral"] + ["fwSSNR", "SSNR"] and [r[:10] for r in rows["spectral_ssnr"]] == rows["spectral"]
    assert heads["all"] == list(eval_cli.CSV_HEADER) + ["estoi", "msstft", "mel", "fwSSNR", "SSNR", "lufs_x_hat", "lufs_x", "lufs_y", "lag_x_hat", "lag_y",
                                                        "pol_x_hat", "pol_y"]
    assert heads["all_off"] == heads["all"][:11] + heads["all"][13:]
    assert [r[:11] + r[13:] for r in rows["all"]] == rows["all_off"]
    assert [m[0] for m in res["ssnr"].means] == list(eval_cli.METRIC_NAMES) + ["fwSSNR", "SSNR"] and res["ssnr"].means[:4] == res["base"].means
    assert [m[0] for m in res["all"].means] == list(eval_cli.METRIC_NAMES) + ["estoi", "msstft", "mel", "fwSSNR", "SSNR"]
    assert caps["ssnr"].out.count("mean =") == 6 and "fwSSNR" in caps["ssnr"].out and caps["all"].out.count("mean =") == 12
    # the 1799-sample triple: NaN in exactly those two columns, and a warning naming the rule
    short = rows["ssnr"][1]
    assert short[-2:] == ["nan", "nan"] and all(v != "nan" for v in short[4:8]) and "enh_1.wav" in caps["ssnr"].err and "1800 samples" in caps["ssnr"].err
    assert res["ssnr"].means[-1][2] == 2 and res["ssnr"].means[-2][2] == 2
    # the wav files are 16-bit: score what was written
    for i in (0, 2):
        r = rows["ssnr"][i]
        h, x = load_mono(r[1], SR).numpy(), load_mono(r[2], SR).numpy()
        assert float(r[-2]) == segsnr.fw_segmental_snr(h, x, SR) and float(r[-1]) == segsnr.segmental_snr(h, x, SR)
        assert -10 < float(r[-1]) < 35 and -10 < float(r[-2]) < 35
    # score(): the column layout; unequal lengths stay NaN everywhere; a Scorer without the field refuses
    assert eval_cli.metric_columns(True, True, True) == eval_cli.METRIC_NAMES + ("estoi", "msstft", "mel", "fwSSNR", "SSNR")
    assert eval_cli.metric_columns(ssnr=True) == eval_cli.METRIC_NAMES + ("fwSSNR", "SSNR") and eval_cli.metric_columns(True, True) == eval_cli.metric_columns(True, True, False)
    sig = [tuple(torch.from_numpy(a) for a in (pair(4800, SR, 5, 15) + (pair(4800, SR, 6, 15)[1],)))]
    bad = sig + [(sig[0][0][:-1], sig[0][1], sig[0][2])]
    v = eval_cli.score(bad, SR, 2, eval_cli.HOST_SCORER, spectral=True, ssnr=True)
    assert v.shape == (2, 8) and np.isnan(v[1]).all() and np.isfinite(v[0]).all()
    assert np.array_equal(v[:1, :6], eval_cli.score(sig, SR, 2, eval_cli.HOST_SCORER, spectral=True))
    with pytest.raises(ValueError):
        eval_cli.score(sig, SR, 2, eval_cli.Scorer(eval_cli.HOST_SCORER.si_sxr, eval_cli.HOST_SCORER.logspec), ssnr=True)
    assert eval_cli.GPU_SCORER.segsnr is not None and eval_cli.HOST_SCORER.segsnr is not None
    assert [f.name for f in __import__("dataclasses").fields(eval_cli.Scorer)][-1] == "segsnr"


def test_match_loudness_and_align_come_first(tmp_path, capsys):
    """--ssnr scores the signals that --align and --match-loudness leave, like the other metrics that are not scale-invariant."""
    from flowdec_amd import eval_cli, loudness, segsnr
    from flowdec_amd.eval_cli import load_mono
    n = 24000                                                                              # 0.5 s: above the 400 ms block of the loudness gate
    h, x = pair(n, SR, 31, 15)
    y = (x + 0.1 * np.random.default_rng(5).standard_normal(n)).astype(np.float32)
    paths = [tmp_path / "clean.wav", tmp_path / "noisy.wav", tmp_path / "enh.wav"]
    for path, s in zip(paths, (x, y, 0.25 * h)):
        write_wav(path, s, SR)
    lst = tmp_path / "triples_list.txt"
    lst.write_text(" ---> ".join(str(q) for q in paths) + "\n")
    got = {}
    for k, extra in (("plain", []), ("matched", ["--match-loudness"])):
        eval_cli.run(["--triples", str(lst), "--out", str(tmp_path / f"{k}.csv"), "--ssnr"] + extra, scorer=eval_cli.HOST_SCORER)
        capsys.readouterr()
        head, rows = read_csv(tmp_path / f"{k}.csv")
        got[k] = [float(rows[0][head.index(c)]) for c in ("fwSSNR", "SSNR")]
    hq, xq = load_mono(str(paths[2]), SR), load_mono(str(paths[0]), SR)
    assert got["plain"] == [segsnr.fw_segmental_snr(hq.numpy(), xq.numpy(), SR), segsnr.segmental_snr(hq.numpy(), xq.numpy(), SR)]
    lufs = loudness.host_loudness([hq, xq], SR, 2)
    hm = loudness.match_loudness(hq, lufs[0], lufs[1]).numpy()
    assert got["matched"] == [segsnr.fw_segmental_snr(hm, xq.numpy(), SR), segsnr.segmental_snr(hm, xq.numpy(), SR)]
    assert got["matched"][1] > got["plain"][1] + 3                                         # a quarter of the level costs SSNR; matched, it is back


def test_parser_flags_of_both_command_lines(monkeypatch):
    from flowdec_amd import enhance_cli, eval_cli
    a = eval_cli.build_parser().parse_args(["--triples", "t", "--out", "o"])
    assert not a.ssnr
    a = eval_cli.build_parser().parse_args(["--triples", "t", "--out", "o", "--ssnr", "--spectral"])
    assert a.ssnr and a.spectral and not a.estoi
    base = ["--ckpt", "c", "--files", "f", "--outdir", "o", "--N", "3"]
    args = enhance_cli.build_parser().parse_args(base + ["--eval", "--eval-ssnr"])
    assert args.eval and args.eval_ssnr and not args.eval_spectral and not enhance_cli.build_parser().parse_args(base + ["--eval"]).eval_ssnr
    seen = []
    monkeypatch.setattr(eval_cli, "run", lambda argv, **kw: seen.append(list(argv)))
    monkeypatch.setattr(torch.cuda, "device", lambda d: __import__("contextlib").nullcontext())
    args.device, args.batch_files = "cuda", 4
    enhance_cli.evaluate_triples(args, "")
    args.eval_match_loudness = True
    enhance_cli.evaluate_triples(args, "")
    args.eval_ssnr = False
    enhance_cli.evaluate_triples(args, "")
    assert seen[0][-1] == "--ssnr" and seen[1][-2:] == ["--match-loudness", "--ssnr"] and seen[2][-1] == "--match-loudness" and seen[0][:-1] == seen[2][:-1]
