"""Pins flowdec_amd.segsnr against the pysepm package, where that is installed: the host functions restate
pysepm.qualityMeasures.fwSNRseg / SNRseg with frameLen=0.03, overlap=0.75 (the reference's fwSSNR and SSNR, flowdec/eval/metrics.py:511-547)
and no test can import pysepm, so the parity with the package itself is UNPINNED until somebody runs this and records the numbers in
MEASUREMENTS.md.  Not run by any test.

Expected differences: the order of a few float64 sums and NumPy's cos / exp against libm's in the window and the bank, 1e-10 dB or so.
Anything above ~1e-9 dB on the seeded clips below is a finding -- first of all the table of the 25 critical bands (this restatement:
seven bands of 70 Hz, band_i = cent_(i+1) - cent_i, the last one 346.136 Hz) and the frame count of fwSNRseg, int(len / skip - win / skip).

    python scripts/pin_segsnr.py [--clips 8]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=8)
    args = ap.parse_args()
    try:
        from pysepm import qualityMeasures
    except ImportError:
        print("pin_segsnr: pysepm is absent here; nothing compared (the parity of flowdec_amd.segsnr with pysepm stays unpinned)")
        return 2
    from flowdec_amd import segsnr
    worst = [0.0, 0.0]
    for i in range(args.clips):
        rng = np.random.default_rng(i)
        sr = (48000, 16000, 8000, 44100)[i % 4]
        n = int(sr * (0.5 + 0.25 * i)) + 13 * i
        t = np.arange(n) / sr
        x = (rng.standard_normal(n) * (0.55 + 0.45 * np.sin(2 * np.pi * 3 * t)) * (np.sin(2 * np.pi * 2.3 * t + 0.3) > -0.8)).astype(np.float32)
        nz = rng.standard_normal(n)
        h = (x + nz * np.sqrt(np.mean(x ** 2.0) / np.mean(nz ** 2)) * 10 ** (-(25 - 5 * i) / 20)).astype(np.float32)
        if i % 2:
            h[n - n // 5:] = 0.0                                             # a silent tail in x_hat only
        ref = (float(qualityMeasures.fwSNRseg(x.astype(np.float64), h.astype(np.float64), sr, frameLen=0.03, overlap=0.75)),
               float(qualityMeasures.SNRseg(x.astype(np.float64), h.astype(np.float64), sr, frameLen=0.03, overlap=0.75)))
        d = segsnr.segsnr_detail(h, x, sr)
        got = (d["fwssnr"], d["ssnr"])
        for k in range(2):
            worst[k] = max(worst[k], abs(got[k] - ref[k]))
        print(f"clip {i}: sr {sr} {n / sr:.2f} s, {d['frames']} frames  fwSSNR pysepm {ref[0]:.12f} flowdec_amd {got[0]:.12f} diff {got[0] - ref[0]:+.3e}   "
              f"SSNR pysepm {ref[1]:.12f} flowdec_amd {got[1]:.12f} diff {got[1] - ref[1]:+.3e}")
    print(f"pin_segsnr: largest |difference| over {args.clips} clips: fwSSNR {worst[0]:.3e} dB, SSNR {worst[1]:.3e} dB "
          f"(pysepm {getattr(__import__('pysepm'), '__version__', '?')})")
    return 0


if __name__ == "__main__":
    sys.exit(main())
