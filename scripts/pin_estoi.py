"""Pins flowdec_amd.metrics.estoi against the pystoi package, where that is installed: the host function restates
pystoi.stoi(x, x_hat, sr, extended=True) (the reference's ESTOI, flowdec/eval/metrics.py:273-283) and no test can import pystoi, so the
parity with the package itself is UNPINNED until somebody runs this and records the numbers in MEASUREMENTS.md.  Not run by any test.

Expected differences: pystoi adds eps * randn before each normalisation (below 1e-12), and draws a random unit vector where a row or
column is exactly zero (this restatement: zeros).  Anything above ~1e-9 on the seeded clips below is a finding.

    python scripts/pin_estoi.py [--clips 8]
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
        import pystoi
    except ImportError:
        print("pin_estoi: pystoi is not importable here; nothing compared (the parity of flowdec_amd.metrics.estoi with pystoi stays unpinned)")
        return 2
    from flowdec_amd import metrics
    worst = 0.0
    for i in range(args.clips):
        rng = np.random.default_rng(i)
        sr = (48000, 16000, 44100, 10000)[i % 4]
        n = int(sr * (1.0 + 0.5 * i))
        t = np.arange(n) / sr
        x = rng.standard_normal(n) * (0.55 + 0.45 * np.sin(2 * np.pi * 3 * t)) * ((np.sin(2 * np.pi * 2.3 * t + 0.3) > -0.8) + 1e-4)
        nz = rng.standard_normal(n)
        y = x + nz * np.sqrt(np.mean(x ** 2) / np.mean(nz ** 2)) * 10 ** (-(20 - 5 * i) / 20)
        np.random.seed(0)                                                      # pystoi's eps * randn
        ref = float(pystoi.stoi(x, y, sr, extended=True))
        got = metrics.estoi(y, x, sr)
        worst = max(worst, abs(got - ref))
        print(f"clip {i}: sr {sr} {n / sr:.1f} s  pystoi {ref:.15f}  flowdec_amd {got:.15f}  diff {got - ref:+.3e}")
    print(f"pin_estoi: largest |difference| over {args.clips} clips = {worst:.3e} (pystoi {getattr(pystoi, '__version__', '?')})")
    return 0


if __name__ == "__main__":
    sys.exit(main())
