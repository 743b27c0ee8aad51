#!/usr/bin/env python
"""Prints flowdec_amd.loudness.integrated_loudness beside pyloudnorm.Meter(48000).integrated_loudness where that package is importable
(it is not available to the tests: parity with it is UNPINNED).  pyloudnorm derives its K-weighting coefficients from
filter parameters and takes its blocks from a length rule of its own, so agreement is expected to a few thousandths of a dB, not to the bit.

    python scripts/pin_loudness.py [--seconds 20]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=20.0)
    args = ap.parse_args()
    from flowdec_amd import loudness
    try:
        import pyloudnorm
    except ImportError:
        print("pyloudnorm is not importable here: nothing to compare (parity stays unpinned)")
        return 0
    meter = pyloudnorm.Meter(48000)
    rng = np.random.default_rng(0)
    n = int(args.seconds * 48000)
    t = np.arange(n) / 48000.0
    cases = {"997 Hz sine, 0 dBFS": np.sin(2 * np.pi * 997 * t), "noise, -20 dB": 0.1 * rng.standard_normal(n),
             "noise, second half 30 dB down": 0.1 * rng.standard_normal(n) * np.where(t < args.seconds / 2, 1.0, 10 ** -1.5)}
    for name, x in cases.items():
        x = x.astype(np.float32)
        ours, theirs = loudness.integrated_loudness(x), meter.integrated_loudness(x.astype(np.float64))
        print(f"{name:32s} flowdec_amd {ours:.6f} LUFS   pyloudnorm {theirs:.6f} LUFS   difference {ours - theirs:+.2e} dB")
    return 0


if __name__ == "__main__":
    sys.exit(main())
