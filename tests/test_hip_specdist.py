"""The spectral distances on the GPU (csrc/specdist.hip) against the float64 yardsticks of flowdec_amd.specdist.

Every bound below is computed from the yardstick's float64 spectra, never from the code under test.

Bnd, per frame: the normwise error bound of a float32 FFT of N points (Higham, ASNA Thm 24.2: about 7 u log2 N ||X||_2 with
||X||_2 = sqrt(N) ||frame||_2), taken over the packed sequence z = w x_hat + i w x, with the factor 16 instead of 7 for the window rounding,
the unpacking and the square root:  Bnd = 16 log2(N) 2^-24 sqrt(N) sqrt(||w x_hat_frame||^2 + ||w x_frame||^2).
Mel: |dM_j| <= sum_f fb[f][j] (2 |X_f| Bnd + Bnd^2) + 2^-22 M_j (the weights' float32 rounding, P = A^2 and the rounding of M to float32).
Log terms: |log10 max(a, c) - log10 max(b, c)| <= |a - b| / (ln 10 max(min(a, b), c)) with min(a, b) replaced by |X| - Bnd.
The sharper gate: per scale the largest magnitude error is at most 16 times that of torch.stft in float32 on the CPU on the same inputs
(another radix, the table's rounding and the packed transform are what the margin is for).

Figures of the first GPU run are in MEASUREMENTS.md "Spectral distances"."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from test_eval_cpu import read_csv, write_wav
from test_specdist_cpu import LENGTHS, SR, make_triples, signals

pytestmark = pytest.mark.gpu

FD_EINVAL = -1
U = 2.0 ** -24
CLAMP = 1e-5


@pytest.fixture(scope="module")
def clips():
    """The five seeded pairs and their float64 detail, computed once and never changed."""
    from flowdec_amd import specdist
    pairs = [signals(n, 40 + i) for i, n in enumerate(LENGTHS)]
    return pairs, [specdist.detail(h, x, SR) for h, x in pairs]


@pytest.fixture(scope="module")
def plan():
    from flowdec_amd import specdist
    return specdist.specdist_plan(SR, "cuda")


def stage(pairs, Lrow=None):
    from flowdec_amd.batching import padded_rows
    Lrow = Lrow or max(len(x) for _, x in pairs)
    rh, lens = padded_rows([torch.from_numpy(h) for h, _ in pairs], Lrow, "cuda")
    rx, _ = padded_rows([torch.from_numpy(x) for _, x in pairs], Lrow, "cuda")
    return rh, rx, lens, Lrow


def distances(plan, pairs, lens_override=None):
    """fd_metrics_specdist on one batch -> (out [B, 2], terms [B, 6, 3]) as host arrays."""
    from flowdec_amd import _lib as L
    lib = L.load()
    rh, rx, lens, Lrow = stage(pairs)
    if lens_override is not None:
        lens = torch.tensor(lens_override, dtype=torch.int32, device="cuda")
    B, k = len(pairs), len(plan.scales)
    nws = lib.fd_metrics_specdist_workspace_bytes(plan.handle, B, Lrow)
    assert nws > 0
    ws = torch.empty(nws, dtype=torch.uint8, device="cuda")
    out = torch.full((B, 2), -7.0, dtype=torch.float64, device="cuda")
    terms = torch.full((B, k, 3), -7.0, dtype=torch.float64, device="cuda")
    L.check(lib.fd_metrics_specdist(plan.handle, L.ptr(rh), L.ptr(rx), L.ptr(lens), B, Lrow, L.ptr(out), L.ptr(terms), L.ptr(ws), nws, L.stream()))
    torch.cuda.synchronize()
    return out.cpu().numpy(), terms.cpu().numpy()


def spectra(plan, pairs, scale):
    from flowdec_amd import _lib as L
    lib = L.load()
    rh, rx, lens, Lrow = stage(pairs)
    n_fft, n_mels, _ = plan.scales[scale]
    B, T, F = len(pairs), 1 + Lrow // (n_fft // 4), n_fft // 2 + 1
    nws = lib.fd_metrics_specdist_workspace_bytes(plan.handle, B, Lrow)
    ws = torch.empty(nws, dtype=torch.uint8, device="cuda")
    mag = [torch.full((B, T, F), float("nan"), dtype=torch.float32, device="cuda") for _ in range(2)]
    mel = [torch.full((B, T, n_mels), float("nan"), dtype=torch.float32, device="cuda") for _ in range(2)]
    L.check(lib.fd_metrics_specdist_spectra(plan.handle, scale, L.ptr(rh), L.ptr(rx), L.ptr(lens), B, Lrow, L.ptr(mag[0]), L.ptr(mag[1]), L.ptr(mel[0]),
                                            L.ptr(mel[1]), L.ptr(ws), nws, L.stream()))
    torch.cuda.synchronize()
    return [m.cpu().numpy() for m in mag], [m.cpu().numpy() for m in mel]


def frame_bound(sc):
    """Bnd [T] of one scale of a clip's detail."""
    n = sc["n_fft"]
    return 16 * math.log2(n) * U * math.sqrt(n) * np.sqrt(sc["energy"])


def mel_bound(sc, sr, which):
    """[T, n_mels]: the bound on |M_gpu - M_f64| of one signal."""
    from flowdec_amd import specdist
    fb = specdist.mel_filterbank(sr, sc["n_fft"], sc["n_mels"])
    X, M = np.abs(sc["spec_" + which]), sc["mel_" + which]
    bnd = frame_bound(sc)[:, None]
    return (2 * X * bnd + bnd ** 2) @ fb + 2.0 ** -22 * M


def log_bound(v, dv):
    """The bound on |2 log10 max(v', c) - 2 log10 max(v, c)| for |v' - v| <= dv."""
    return 2 * dv / (math.log(10) * np.maximum(v - dv, CLAMP))


def metric_bounds(d, sr):
    """-> (bound on |msstft_gpu - msstft_f64|, bound on |mel_gpu - mel_f64|) of one clip's detail: the per-bin bounds pushed through the
    terms (a mean of bounded differences is bounded by the mean of the bounds), plus 1e-12 relative for the float64 sums of either side."""
    b_st, b_mel = 0.0, 0.0
    for sc in d["scales"]:
        bnd = frame_bound(sc)[:, None]
        if sc["stft"]:
            A, R = np.abs(sc["spec_hat"]), np.abs(sc["spec_x"])
            b_st += float(np.mean(log_bound(A, bnd) + log_bound(R, bnd))) + float(np.mean(2 * bnd + 0 * A))
        if sc["n_mels"]:
            b_mel += float(np.mean(log_bound(sc["mel_hat"], mel_bound(sc, sr, "hat")) + log_bound(sc["mel_x"], mel_bound(sc, sr, "x"))))
    return b_st + 1e-12 * d["msstft"], b_mel + 1e-12 * d["mel"]


def torch_f32_error(pairs, dets, scale):
    """The largest |torch.stft float32 magnitude - float64 magnitude| over the batch at one scale: the reference library's own error."""
    worst = 0.0
    for (h, x), d in zip(pairs, dets):
        sc = d["scales"][scale]
        n = sc["n_fft"]
        for sig, key in ((h, "spec_hat"), (x, "spec_x")):
            S = torch.stft(torch.from_numpy(sig), n, hop_length=n // 4, win_length=n, window=torch.hann_window(n, periodic=True), center=True,
                           pad_mode="reflect", return_complex=True).abs().numpy().T.astype(np.float64)
            worst = max(worst, float(np.max(np.abs(S - np.abs(sc[key])))))
    return worst


@pytest.mark.parametrize("scale", range(6))
def test_spectra_within_the_fft_bound(clips, plan, scale):
    pairs, dets = clips
    (mag_h, mag_x), (mel_h, mel_x) = spectra(plan, pairs, scale)
    n_fft, n_mels, _ = plan.scales[scale]
    worst, worst_rel, worst_mel = 0.0, 0.0, 0.0
    for b, d in enumerate(dets):
        sc = d["scales"][scale]
        Tb = 1 + LENGTHS[b] // (n_fft // 4)
        assert sc["spec_x"].shape == (Tb, n_fft // 2 + 1) and 3 <= Tb <= 282
        bnd = frame_bound(sc)[:, None]
        for got, key, gmel, which in ((mag_h, "spec_hat", mel_h, "hat"), (mag_x, "spec_x", mel_x, "x")):
            err = np.abs(got[b, :Tb].astype(np.float64) - np.abs(sc[key]))
            assert np.all(err <= bnd), (n_fft, b, float(np.max(err / bnd)))
            assert np.all(got[b, Tb:] == 0) and np.all(gmel[b, Tb:] == 0)                 # frames the clip does not have
            worst, worst_rel = max(worst, float(err.max())), max(worst_rel, float(np.max(err / bnd)))
            merr = np.abs(gmel[b, :Tb].astype(np.float64) - sc["mel_" + which])
            mb = mel_bound(sc, SR, which)
            assert np.all(merr <= mb), (n_fft, b, float(np.max(merr / mb)))
            worst_mel = max(worst_mel, float(np.max(merr / mb)))
    ref = torch_f32_error(pairs, dets, scale)
    print(f"specdist N {n_fft}: max |mag err| {worst:.3e} = {worst_rel:.4f} Bnd = {worst / ref:.2f} x torch.stft float32 ({ref:.3e}); "
          f"mel err at most {worst_mel:.4f} of its bound")
    assert worst <= 16 * ref, (n_fft, worst, ref)


def test_metrics_within_the_propagated_bound(clips, plan):
    pairs, dets = clips
    out, terms = distances(plan, pairs)
    for b, d in enumerate(dets):
        b_st, b_mel = metric_bounds(d, SR)
        e_st, e_mel = abs(out[b, 0] - d["msstft"]), abs(out[b, 1] - d["mel"])
        print(f"specdist clip {LENGTHS[b]}: msstft {out[b, 0]:.9f} err {e_st:.2e} (rel {e_st / d['msstft']:.1e}, bound {b_st:.2e}); "
              f"mel {out[b, 1]:.9f} err {e_mel:.2e} (rel {e_mel / d['mel']:.1e}, bound {b_mel:.2e})")
        assert e_st <= b_st and e_mel <= b_mel
        for s, sc in enumerate(d["scales"]):
            assert np.allclose(terms[b, s], sc["terms"], rtol=0, atol=max(b_st, b_mel))
            if not sc["stft"]:
                assert terms[b, s, 0] == 0.0 and terms[b, s, 1] == 0.0
        assert abs(out[b, 0] - terms[b, :, :2].sum()) < 1e-13 and abs(out[b, 1] - terms[b, :, 2].sum()) < 1e-13


def test_batch_invariance_bit_for_bit(clips, plan):
    from flowdec_amd import specdist
    pairs, _ = clips
    out5, terms5 = distances(plan, pairs)
    rev_out, rev_terms = distances(plan, pairs[::-1])
    assert np.array_equal(rev_out[::-1], out5) and np.array_equal(rev_terms[::-1], terms5)                 # at another row
    for b, pair in enumerate(pairs):
        o1, t1 = distances(plan, [pair])                                                                     # alone
        o2, t2 = distances(plan, [pair, pairs[-1]])                                                          # next to a 9001-sample neighbour
        assert np.array_equal(o1[0], out5[b]) and np.array_equal(t1[0], terms5[b])
        assert np.array_equal(o2[0], out5[b]) and np.array_equal(t2[0], terms5[b])
    hs, xs = [h for h, _ in pairs], [x for _, x in pairs]
    a = specdist.spectral_distances_batch(hs, xs, SR, batch=2)
    c, tc = specdist.spectral_distances_batch(hs, xs, SR, batch=8, return_terms=True)
    assert a.shape == (5, 2) and np.array_equal(a, c) and np.array_equal(c, out5) and np.array_equal(tc, terms5)
    with pytest.raises(ValueError, match="clip 1 has 2048 samples"):
        specdist.spectral_distances_batch([hs[2], hs[2][:2048]], [xs[2], xs[2][:2048]], SR)


def test_identity_and_scaling(clips, plan):
    """x_hat = x scores exactly 0.  Scaling both signals by 2 doubles every magnitude and quadruples every mel value exactly (operator level,
    all six scales), doubles every stft mag term exactly and leaves the bits of every log term unchanged -- where the metric itself has that
    property: a value under the clamp 1e-5 does not scale, so a log term is compared at the (clip, scale) pairs whose float64 values all lie
    above twice the clamp (the float32 error at such small values is far below 1e-5; were it not, this test would fail, not pass).  That
    is known from the yardstick alone: every stft term (the smallest |X| of these clips is 5e-5) and 26 of the 30 mel terms (one value of
    the 4095-sample clip at N = 512 is 3.7e-6, three other pairs have one between 1.6e-5 and 1.8e-5)."""
    pairs, dets = clips
    same = [(x, x) for _, x in pairs]
    out, terms = distances(plan, same)
    assert np.all(out == 0.0) and np.all(terms == 0.0)                                                      # exactly 0, every term
    doubled = [(2 * h, 2 * x) for h, x in pairs]
    for scale in range(6):
        (m1h, m1x), (l1h, l1x) = spectra(plan, pairs, scale)
        (m2h, m2x), (l2h, l2x) = spectra(plan, doubled, scale)
        assert np.array_equal(m2h, 2 * m1h) and np.array_equal(m2x, 2 * m1x) and np.array_equal(l2h, 4 * l1h) and np.array_equal(l2x, 4 * l1x)
    out1, terms1 = distances(plan, pairs)
    out2, terms2 = distances(plan, doubled)
    assert np.array_equal(terms2[:, :, 1], 2 * terms1[:, :, 1]) and np.all(terms1[:, 2:, 1] > 0)                  # the magnitude terms double
    compared = [0, 0]
    for b, d in enumerate(dets):
        for s, sc in enumerate(d["scales"]):
            if sc["stft"]:
                assert min(np.min(np.abs(sc["spec_hat"])), np.min(np.abs(sc["spec_x"]))) > 2 * CLAMP
                assert terms2[b, s, 0] == terms1[b, s, 0] and terms1[b, s, 0] > 0
                compared[0] += 1
            if min(np.min(sc["mel_hat"]), np.min(sc["mel_x"])) > 2 * CLAMP:
                assert terms2[b, s, 2] == terms1[b, s, 2] and terms1[b, s, 2] > 0
                compared[1] += 1
            else:
                assert abs(terms2[b, s, 2] - terms1[b, s, 2]) < 5e-3          # a few clamped values of T_b x n_mels move the mean little
    assert compared == [20, 26]


def test_refusals_leave_the_outputs_untouched(clips, plan):
    from flowdec_amd import _lib as L
    lib = L.load()
    pairs, _ = clips
    err = lambda: lib.fd_last_error().decode()
    rh, rx, lens, Lrow = stage(pairs)
    B = len(pairs)
    nws = lib.fd_metrics_specdist_workspace_bytes(plan.handle, B, Lrow)
    assert lib.fd_metrics_specdist_workspace_bytes(plan.handle, 0, Lrow) == 0 and lib.fd_metrics_specdist_workspace_bytes(plan.handle, 65536, Lrow) == 0
    assert lib.fd_metrics_specdist_workspace_bytes(plan.handle, B, 2048) == 0 and lib.fd_metrics_specdist_workspace_bytes(plan.handle, B, 2049) > 0
    ws = torch.empty(nws, dtype=torch.uint8, device="cuda")
    out = torch.full((B, 2), -7.0, dtype=torch.float64, device="cuda")
    terms = torch.full((B, 6, 3), -7.0, dtype=torch.float64, device="cuda")
    mag = torch.full((B, 1 + Lrow // 32, 65), -7.0, dtype=torch.float32, device="cuda")
    p = L.ptr
    call = lambda plan_=plan.handle, xh=p(rh), x=p(rx), ln=p(lens), B_=B, L_=Lrow, o=p(out), w=p(ws), n=nws: \
        lib.fd_metrics_specdist(plan_, xh, x, ln, B_, L_, o, p(terms), w, n, L.stream())
    assert call(xh=None) == FD_EINVAL and "null pointer" in err()
    assert call(o=None) == FD_EINVAL and "null pointer" in err()
    assert call(B_=0) == FD_EINVAL and "bad batch B 0" in err()
    assert call(L_=2048) == FD_EINVAL and "cannot be reflect-padded" in err()
    assert call(n=nws - 1) == FD_EINVAL and "workspace too small" in err()
    spec = lambda scale=0, mh=p(mag), n=nws, mel=None: lib.fd_metrics_specdist_spectra(plan.handle, scale, p(rh), p(rx), p(lens), B, Lrow, mh, p(mag), mel,
                                                                                       None, p(ws), n, L.stream())
    assert spec(mh=None) == FD_EINVAL and "null pointer" in err()
    assert spec(scale=6) == FD_EINVAL and "scale 6" in err()
    assert spec(n=nws - 1) == FD_EINVAL and "workspace too small" in err()
    assert spec(mel=p(mag)) == FD_EINVAL and "go together" in err()
    torch.cuda.synchronize()
    assert torch.all(out == -7.0) and torch.all(terms == -7.0) and torch.all(mag == -7.0)
    # a device length the host cannot see: 2048 (too short) and Lrow + 1 (beyond the row) give NaN for that clip alone
    good_out, good_terms = distances(plan, pairs)
    for bad in (2048, Lrow + 1, 0, -5):
        ln = list(LENGTHS)
        ln[1] = bad
        o, t = distances(plan, pairs, lens_override=ln)
        assert np.all(np.isnan(o[1])) and np.all(np.isnan(t[1]))
        keep = [0, 2, 3, 4]
        assert np.array_equal(o[keep], good_out[keep]) and np.array_equal(t[keep], good_terms[keep])


def test_eval_cli_spectral_end_to_end(tmp_path, capsys):
    from flowdec_amd import eval_cli, specdist
    from flowdec_amd.eval_cli import load_mono
    lst = make_triples(tmp_path, [2400, 9600, 5000, 2048], seed=7)                  # 0.05 s .. 0.2 s, and one under the 2049-sample rule
    gpu, host = tmp_path / "gpu.csv", tmp_path / "host.csv"
    r_gpu = eval_cli.run(["--triples", str(lst), "--out", str(gpu), "--batch-files", "3", "--spectral"])
    cap = capsys.readouterr()
    eval_cli.run(["--triples", str(lst), "--out", str(host), "--batch-files", "3", "--spectral"], scorer=eval_cli.HOST_SCORER)
    (hg, rg), (hh, rh) = read_csv(gpu), read_csv(host)
    assert hg == hh == list(eval_cli.CSV_HEADER) + ["msstft", "mel"] and len(rg) == 4
    assert cap.out.count("mean =") == 6 and "msstft" in cap.out and "mel " in cap.out and "2049" in cap.err
    assert rg[3][-2:] == ["nan", "nan"] and rh[3][-2:] == ["nan", "nan"] and r_gpu.means[-1][2] == 3
    for i in range(3):
        h, x = load_mono(rg[i][1], SR).numpy(), load_mono(rg[i][2], SR).numpy()
        b_st, b_mel = metric_bounds(specdist.detail(h, x, SR), SR)
        assert abs(float(rg[i][-2]) - float(rh[i][-2])) <= b_st and abs(float(rg[i][-1]) - float(rh[i][-1])) <= b_mel
        assert float(rg[i][-2]) > 0 and float(rg[i][-1]) > 0
