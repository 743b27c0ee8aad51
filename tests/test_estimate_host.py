"""Host side of the parameter estimator (flowdec_amd/estimate.py, flowdec_amd/estimate_cli.py): everything that needs no GPU.

* select_pairs / crop_or_pad_pair draw what the reference script drew (golden g32_estimate_params.npz: its selected lines and crop starts);
* the corpus generator (tests/estimate_corpus.py) gives the bytes the fixture was made from;
* the output file naming rule for the four flag combinations; a coded file shorter than the clean one raises;
* quantile_position + lerp on two order statistics give np.quantile's bits on float32 (and float64) arrays;
* the --compare-ckpt arithmetic on a synthetic checkpoint dict, and the command line around a stubbed estimate_params.
"""
import argparse
import os

import numpy as np
import pytest
import torch

import estimate_corpus as EC
from conftest import load_golden


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("estimate_corpus"))
    return d, EC.build(d)


def test_corpus_hashes_match_fixture(corpus):
    g = load_golden("g32_estimate_params.npz")
    assert EC.hashes(corpus[0]) == [str(h) for h in g["hashes"]]
    n = np.array(EC.X_LENGTHS)
    assert len(n) == 12 and n.min() == 48000 and n.max() == 153600 and (n == 96000).sum() == 1 and (n < 96000).sum() >= 3 and (n > 96000).sum() >= 3
    assert len(EC.Y_EXTRA) == 2


def test_selection_and_crops_reproduce_the_reference(corpus):
    from flowdec_amd import estimate as E
    from flowdec_amd.eval_cli import load_mono
    g = load_golden("g32_estimate_params.npz")
    with open(corpus[1]) as f:
        lines = [l.strip() for l in f.readlines()]
    idx, pairs = E.select_pairs(lines, 8, 302, EC.DELIM)
    assert idx == g["sel"].tolist()
    starts = []
    for i, (fx, fy) in zip(idx, pairs):
        assert os.path.basename(fx) == EC.names(i)[0] and os.path.basename(fy) == EC.names(i)[1]
        x, y = load_mono(fx, 48000), load_mono(fy, 48000)
        assert x.numel() == EC.X_LENGTHS[i] and y.numel() == EC.X_LENGTHS[i] + EC.Y_EXTRA.get(i, 0)
        xc, yc, start = E.crop_or_pad_pair(x, y, 96000, name=fx)
        assert xc.shape == yc.shape == (96000,)
        if start is None:
            n = min(x.numel(), 96000)
            assert torch.equal(xc[:n], x[:n]) and torch.equal(yc[:n], y[:n]) and not xc[n:].any() and not yc[n:].any()
        else:
            assert torch.equal(xc, x[start:start + 96000]) and torch.equal(yc, y[start:start + 96000])
        starts.append(-1 if start is None else start)
    assert starts == g["crop"].tolist()
    assert sum(s >= 0 for s in starts) >= 2 and sum(EC.X_LENGTHS[i] < 96000 for i in idx) >= 2 and any(i in EC.Y_EXTRA for i in idx)


def test_select_pairs_refusals():
    from flowdec_amd import estimate as E
    with pytest.raises(ValueError, match="3 samples asked of a list of 2"):
        E.select_pairs(["a ---> b", "c ---> d"], 3, 1)
    with pytest.raises(ValueError, match="is no `clean ---> coded` pair"):
        E.select_pairs(["a,b"], 1, 1)


def test_short_coded_signal_raises():
    from flowdec_amd import estimate as E
    with pytest.raises(ValueError, match="clean_07.wav: the coded signal has 999 samples, fewer than the clean signal's 1000"):
        E.crop_or_pad_pair(torch.zeros(1000), torch.zeros(999), 500, name="clean_07.wav")
    E.crop_or_pad_pair(torch.zeros(1000), torch.zeros(1001), 500)          # a longer y is cut


def test_output_path_rule():
    from flowdec_amd import estimate_cli as CLI
    base = dict(pairs_file="/data/set/pairs.txt", nfft=1534, hop=384, alpha=0.3, seed=302)
    stem = "/data/set/flowdec_autoparams_nfft1534_hop384_alpha0.3_seed302"
    cases = [(dict(n_samples=2500, per_band=False, outfile_suffix=None), ""), (dict(n_samples=8, per_band=False, outfile_suffix=None), "_n8"),
             (dict(n_samples=2500, per_band=True, outfile_suffix=None), "_perband"), (dict(n_samples=8, per_band=True, outfile_suffix="v2"), "_n8_perband_v2")]
    for flags, suffix in cases:
        txt, npy = CLI.outfile_paths(argparse.Namespace(**base, **flags))
        assert txt == stem + suffix + ".txt" and npy == stem + suffix + "sigy_perband.npy"
    assert CLI.outfile_paths(argparse.Namespace(**base, **cases[2][0]))[1].endswith("_perbandsigy_perband.npy")
    a = CLI.build_parser().parse_args(["--pairs-file", "p.txt", "--alpha", "0.5", "--nfft", "510", "--hop", "128"])
    assert (a.sr, a.n_samples, a.sample_duration, a.seed, a.qx, a.qrmse, a.per_band, a.overwrite, a.device, a.delim) == \
        (48000, 2500, 2.0, 302, 0.997, 0.997, False, False, 0, " ---> ")
    assert CLI.outfile_paths(a)[0] == "flowdec_autoparams_nfft510_hop128_alpha0.5_seed302.txt"


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_two_order_statistics_give_np_quantile(dtype):
    from flowdec_amd import estimate as E
    rng = np.random.default_rng(5)
    for n in (1, 2, 3, 10, 257, 1000, 65537, 3000001):
        a = (np.abs(rng.standard_normal(n)) ** 0.3).astype(dtype)
        for q in (0.0, 0.25, 0.5, 0.997, 0.9999, 1.0):
            lo, hi, gamma = E.quantile_position(n, q, dtype)
            assert 0 <= lo <= hi <= n - 1 and hi - lo <= 1
            part = np.partition(a, sorted({lo, hi}))
            got, want = E.lerp(part[lo], part[hi], gamma), np.quantile(a, q)
            assert got.dtype == want.dtype == dtype and got.tobytes() == want.tobytes(), (n, q, got, want)


def test_rmses_from_band_sq():
    from flowdec_amd import estimate as E
    rng = np.random.default_rng(6)
    d = (rng.standard_normal((3, 5, 7)) + 1j * rng.standard_normal((3, 5, 7))).astype(np.complex64)        # [n, F, T]
    band = (d.real.astype(np.float64) ** 2 + d.imag.astype(np.float64) ** 2).sum(-1)
    per = E.rmses_from_band_sq(band, 7, True)
    assert per.dtype == np.float32 and per.shape == (3, 5)
    np.testing.assert_allclose(per, np.linalg.norm(d, axis=-1) / 5 ** 0.5, rtol=3e-7)          # / sqrt(F): the reference's divisor
    glob = E.rmses_from_band_sq(band, 7, False)
    assert glob.dtype == np.float64 and glob.shape == (3,)
    np.testing.assert_allclose(glob, np.linalg.norm(d.reshape(3, -1), axis=-1) / 35 ** 0.5, rtol=3e-7)


def test_compare_ckpt_arithmetic():
    from flowdec_amd import estimate as E, estimate_cli as CLI
    rng = np.random.default_rng(7)
    raw = (0.2 + 0.05 * rng.random(768)).astype(np.float32)
    res = E.EstimateResult(beta=0.36, abs_quantile_x=1 / 0.36, max_abs_x=3.7, sigma_y=raw, rmse_quantile=3 * raw, rmse_max=3 * raw, rmses=raw[None])
    sm = CLI.smoothed(raw, 3, 1)
    assert sm.shape == (768,) and sm.dtype == np.float64 and np.abs(np.diff(sm)).max() < np.abs(np.diff(raw)).max() / 3
    # a checkpoint whose curve IS the smoothed estimate, scaled by 1.25: beta 0.33 from the config, distance 0.2
    ckpt = {"hyper_parameters": {"model": {"feature_extractor": {"beta": 0.33}, "sigma_y": {"kernel_bandwidth": 3, "factor": 1}}},
            "state_dict": {"sigma_y": torch.from_numpy(1.25 * sm).unsqueeze(-1)}}
    beta, sig, bw, factor = CLI.ckpt_params(ckpt)
    assert (beta, bw, factor) == (0.33, 3.0, 1.0) and sig.shape == (768,)
    lines = CLI.compare_with_ckpt(res, ckpt)
    assert lines[0] == "=== Checkpoint ===" and "checkpoint 0.3300, estimate 0.3600 (estimate / checkpoint = 1.091)" in lines[1]
    assert "relative L2 distance 0.2000" in lines[2] and "768 bands" in lines[2]
    # the EMA weights win; scalars compare as a ratio; no hyper_parameters: the default beta
    ck2 = {"state_dict": {"sigma_y": torch.tensor(0.5)}, "_pl_ema_state_dict": {"sigma_y": torch.tensor(0.66)}}
    res2 = E.EstimateResult(beta=0.33, abs_quantile_x=3.03, max_abs_x=3.7, sigma_y=0.33, rmse_quantile=0.99, rmse_max=1.0, rmses=np.ones(2))
    lines = CLI.compare_with_ckpt(res2, ck2)
    assert "checkpoint 0.3300, estimate 0.3300" in lines[1] and "checkpoint 0.6600, estimate 0.3300 (estimate / checkpoint = 0.500)" in lines[2]
    assert "--per-band" in CLI.compare_with_ckpt(res2, ckpt)[2] and "--per-band" in CLI.compare_with_ckpt(res, ck2)[2]
    assert "holds none" in CLI.compare_with_ckpt(res2, {"state_dict": {}})[2]


def test_result_lines_formats():
    from flowdec_amd import estimate as E, estimate_cli as CLI
    g = load_golden("g32_estimate_params.npz")
    a = argparse.Namespace(qx=0.997, qrmse=0.997, per_band=False)
    res = E.EstimateResult(beta=float(g["beta_f32"]), abs_quantile_x=float(g["q_x_f32"]), max_abs_x=float(g["max_x_f32"]), sigma_y=float(g["sigma_y_f32"]),
                           rmse_quantile=float(g["rmse_q_f32"]), rmse_max=float(g["rmse_max_f32"]), rmses=g["rmses_f32"])
    assert CLI.result_lines(a, res, None) == [str(l) for l in g["lines_global"]]
    a.per_band = True
    assert CLI.result_lines(a, res, "{DIR}/c.npy")[0] == str(g["lines_perband"][0])
    assert EC.printed_numbers(CLI.result_lines(a, res, "/tmp/1.5/c.npy")) == EC.printed_numbers([str(l) for l in g["lines_perband"]]) == ["2.748", "3.763", "0.36"]


def test_cli_compare_ckpt_end_to_end_with_a_stub_estimate(corpus, tmp_path, monkeypatch, capsys):
    """The command line around the estimate (selection, loading, cropping, files, --compare-ckpt) with estimate_params replaced by a stub
    that checks what it is handed: no GPU is needed for any of it."""
    from flowdec_amd import estimate as E, estimate_cli as CLI
    g = load_golden("g32_estimate_params.npz")
    pairs = tmp_path / "pairs.txt"
    pairs.write_text(open(corpus[1]).read())
    curve = np.linspace(0.1, 0.3, 768).astype(np.float32)
    seen = {}

    def stub(xs, ys, **kw):
        assert len(xs) == len(ys) == 8 and all(x.shape == y.shape == (48000,) for x, y in zip(xs, ys))       # --sample-duration 1 sets the crop
        seen.update(kw)
        return E.EstimateResult(beta=0.5, abs_quantile_x=2.0, max_abs_x=3.0, sigma_y=curve, rmse_quantile=3 * curve, rmse_max=3 * curve,
                                rmses=np.ones((8, 768), np.float32))

    monkeypatch.setattr(E, "estimate_params", stub)
    torch.save({"hyper_parameters": {"model": {"feature_extractor": {"beta": 0.25}}}, "state_dict": {"sigma_y": torch.from_numpy(CLI.smoothed(curve, 3, 1))[:, None]}},
               tmp_path / "m.ckpt")
    res = CLI.run(["--pairs-file", str(pairs), "--alpha", "0.3", "--nfft", "1534", "--hop", "384", "--n-samples", "8", "--per-band", "--sample-duration", "1",
                   "--outfile-suffix", "v2", "--compare-ckpt", str(tmp_path / "m.ckpt")])
    assert res is not None and seen == dict(alpha=0.3, n_fft=1534, hop=384, qx=0.997, qrmse=0.997, per_band=True, batch_pairs=64, device="cuda:0")
    stem = "flowdec_autoparams_nfft1534_hop384_alpha0.3_seed302_n8_perband_v2"
    assert np.array_equal(np.load(tmp_path / (stem + "sigy_perband.npy")), curve)
    out = capsys.readouterr().out.splitlines()
    assert out[2] == "=== Results ===" and out[3] == "   \tq0.997( |x|  ) = 2.000, max( |x|  ) = 3.000"
    assert out[4] == f"-->\tbeta=0.50, sigma_y=<written to {tmp_path / (stem + 'sigy_perband.npy')}>"
    assert out[5] == "=== Checkpoint ===" and "checkpoint 0.2500, estimate 0.5000 (estimate / checkpoint = 2.000)" in out[6]
    assert "relative L2 distance 0.0000" in out[7]
    assert (tmp_path / (stem + ".txt")).read_text().splitlines() == out[:5]               # the comparison is printed, not filed
    assert g["sel"].tolist() == E.select_pairs([l.strip() for l in open(pairs)], 8, 302)[0]
