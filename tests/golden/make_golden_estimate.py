#!/usr/bin/env python
"""Golden g32_estimate_params.npz: the reference's scripts/estimate_flowdec_params.py run on the integer corpus of tests/estimate_corpus.py.
Runs only where the reference is present; none of its code travels, only the numbers written here.

Route taken: the script's REAL `__main__` through runpy.run_path (not a restatement), with make_golden.py's import stubs and two more:
  * torchaudio.load -> flowdec_amd.audio.load_wav (torchaudio is not installed; the corpus is PCM16 at 48 kHz, so no resampling runs);
  * Module.to / Tensor.to send `cuda:*` device strings to the CPU (the script hard-codes device=f'cuda:{args.device}').
Four runs at --alpha 0.3 --nfft 1534 --hop 384 --n-samples 8 --seed 302: global and --per-band, each in float32 (the script as it is) and
with every tensor in float64 (the wav reader returns float64 and torch's default dtype is float64, so the window, the transform, the
compression and NumPy's quantiles all run in double).  |float32 - float64| is the reference's own error: the tests' tolerance.

np.random.randint is wrapped to record the crop starts; the selected lines are read back from the script's globals.  The fixture holds
the selected line indices, the crop starts (-1: none drawn), the result numbers and the [768] curve of the float32 and the float64 runs,
the printed result lines of the float32 runs (directory replaced by {DIR}), and the sha256 of each generated wav.

A number printed with d decimals must not lie within 2e-3 units of its last printed digit of a rounding boundary (else the GPU path's
last-place differences could print another digit): asserted here, so the tests may compare the printed strings.

    python tests/golden/make_golden_estimate.py     # writes tests/golden/g32_estimate_params.npz
"""
import contextlib
import io
import os
import runpy
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as MG  # noqa: E402
import estimate_corpus as EC  # noqa: E402

SCRIPT = os.path.join(MG.REF, "scripts", "estimate_flowdec_params.py")
ARGS = ["--alpha", "0.3", "--nfft", "1534", "--hop", "384", "--n-samples", "8", "--seed", "302"]


def _cpu(v):
    return "cpu" if isinstance(v, str) and v.startswith("cuda") else v


@contextlib.contextmanager
def patched(double: bool):
    from flowdec_amd.audio import load_wav
    ta = sys.modules["torchaudio"]

    def load(path):
        au, fs = load_wav(path)
        return (au.double() if double else au), fs

    starts = []
    mod_to, ten_to, randint, dflt = torch.nn.Module.to, torch.Tensor.to, np.random.randint, torch.get_default_dtype()

    def rec_randint(*a, **k):
        v = randint(*a, **k)
        starts.append(int(v))
        return v

    ta.load = load
    torch.nn.Module.to = lambda self, *a, **k: mod_to(self, *[_cpu(v) for v in a], **{n: _cpu(v) for n, v in k.items()})
    torch.Tensor.to = lambda self, *a, **k: ten_to(self, *[_cpu(v) for v in a], **{n: _cpu(v) for n, v in k.items()})
    np.random.randint = rec_randint
    torch.set_default_dtype(torch.float64 if double else torch.float32)
    try:
        yield starts
    finally:
        torch.nn.Module.to, torch.Tensor.to, np.random.randint = mod_to, ten_to, randint
        torch.set_default_dtype(dflt)


def run_reference(per_band: bool, double: bool):
    """-> dict of what one run of the script's __main__ computed and printed."""
    with tempfile.TemporaryDirectory() as d:
        pairs = EC.build(d)
        argv = [SCRIPT, "--pairs-file", pairs] + ARGS + (["--per-band"] if per_band else [])
        old_argv, buf = sys.argv, io.StringIO()
        sys.argv = argv
        try:
            with patched(double) as starts, contextlib.redirect_stdout(buf):
                g = runpy.run_path(SCRIPT, run_name="__main__")
        finally:
            sys.argv = old_argv
        with open(pairs) as f:
            lines = [l.strip() for l in f]
        index = {l.split(EC.DELIM)[0]: i for i, l in enumerate(lines)}
        sel = [index[p] for p in g["batch_x_files"]]
        # the starts in list order: one draw per selected pair whose x is longer than the target
        it = iter(starts)
        crop = [next(it) if EC.X_LENGTHS[i] > 96000 else -1 for i in sel]
        assert next(it, None) is None
        want_dtype = torch.complex128 if double else torch.complex64
        assert g["all_bins_x"].dtype == want_dtype, g["all_bins_x"].dtype
        out = {"sel": np.array(sel), "crop": np.array(crop), "q_x": float(g["abs_quantile_x"]), "max_x": float(g["all_bins_x"].abs().max()),
               "beta": float(1 / g["abs_quantile_x"])}
        text = buf.getvalue().splitlines()
        res = text[text.index("=== Results ===") + 1:]
        out["lines"] = [l.replace(d, "{DIR}") for l in res]
        if per_band:
            curve = np.load(g["per_band_outfile_path"])
            assert curve.shape == (768,) and curve.dtype == (np.float64 if double else np.float32), (curve.shape, curve.dtype)
            assert os.path.basename(g["per_band_outfile_path"]).endswith("_n8_perbandsigy_perband.npy")
            out["curve"] = curve
            out["rmses"] = np.asarray(g["rmses_per_band"])
        else:
            out["rmse_q"], out["rmse_max"], out["sigma_y"] = float(g["rmse_quantile"]), float(np.max(g["rmses"])), float(g["rmse_quantile"] / 3)
            out["rmses"] = np.asarray(g["rmses"])
        out["hashes"] = EC.hashes(d)
        return out


def clear_of_boundary(value: float, decimals: int) -> None:
    u = value * 10 ** decimals
    frac = u - np.floor(u)
    assert abs(frac - 0.5) >= 2e-3, f"{value!r} printed with {decimals} decimals lies {abs(frac - 0.5):.2e} last-digit units from a rounding boundary"


def main():
    MG._install_stubs()
    runs = {(pb, dbl): run_reference(pb, dbl) for pb in (False, True) for dbl in (False, True)}
    g32, g64, p32, p64 = runs[False, False], runs[False, True], runs[True, False], runs[True, True]
    for r in runs.values():
        assert np.array_equal(r["sel"], g32["sel"]) and np.array_equal(r["crop"], g32["crop"]) and r["hashes"] == g32["hashes"]
    for r in (g32, p32):
        clear_of_boundary(r["q_x"], 3); clear_of_boundary(r["max_x"], 3); clear_of_boundary(r["beta"], 2)
    clear_of_boundary(g32["rmse_q"], 3); clear_of_boundary(g32["rmse_max"], 3); clear_of_boundary(g32["sigma_y"], 2)
    assert (p32["q_x"], p32["max_x"]) == (g32["q_x"], g32["max_x"])          # the two runs see the same clean spectra
    out = {"sel": g32["sel"], "crop": g32["crop"], "hashes": np.array(g32["hashes"]),
           "lines_global": np.array(g32["lines"]), "lines_perband": np.array(p32["lines"])}
    for tag, g, p in (("f32", g32, p32), ("f64", g64, p64)):
        for k in ("q_x", "max_x", "beta", "rmse_q", "rmse_max", "sigma_y"):
            out[f"{k}_{tag}"] = np.float64(g[k])
        out[f"rmses_{tag}"] = np.asarray(g["rmses"], np.float64)
        out[f"curve_{tag}"] = np.asarray(p["curve"], np.float64)
    for k in sorted(out):
        v = out[k]
        print(k, v if v.size <= 8 else f"{v.dtype}{list(v.shape)} mean {v.astype(np.float64).mean() if v.dtype.kind == 'f' else ''}")
    for k in ("q_x", "max_x", "beta", "rmse_q", "rmse_max", "sigma_y"):
        print(f"|f32 - f64| / |f64| {k}: {abs(out[k + '_f32'] - out[k + '_f64']) / abs(out[k + '_f64']):.3e}")
    print("curve: max rel", np.max(np.abs(out["curve_f32"] - out["curve_f64"]) / np.abs(out["curve_f64"])))
    np.savez_compressed(os.path.join(HERE, "g32_estimate_params.npz"), **out)


if __name__ == "__main__":
    main()
