"""Pins flowdec_amd.specdist.mel_filterbank against torchaudio, where that is installed: the reference's MelSpectrogramLoss
(flowdec/losses.py) builds its bank with torchaudio.functional.melscale_fbanks(n_freqs, 0, sr // 2, n_mels, sr, norm="slaney",
mel_scale="htk") in float32, this project restates the formulas in float64, and no test can import torchaudio, so the parity with the
package itself is UNPINNED until somebody runs this and records the numbers in MEASUREMENTS.md.  Not run by any test.

Expected differences: torchaudio's linspace, log10 and pow run in float32, so a weight differs by some float32 ulps of the filter's peak;
anything above ~1e-5 of the peak, or a weight that is zero on one side only away from a filter's edge, is a finding.  The mel distance on a
seeded pair is printed with both banks as well.

    python scripts/pin_mel.py [--sr 48000]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sr", type=int, default=48000)
    args = ap.parse_args()
    try:
        import torchaudio
    except ImportError:
        print("pin_mel: torchaudio is not importable here; nothing compared (the parity of flowdec_amd.specdist.mel_filterbank with "
              "torchaudio stays unpinned)")
        return 2
    from flowdec_amd import specdist
    worst = 0.0
    banks = {}
    for n_fft, n_mels in specdist.MEL_SCALES:
        ref = torchaudio.functional.melscale_fbanks(n_freqs=n_fft // 2 + 1, f_min=0.0, f_max=float(args.sr // 2), n_mels=n_mels, sample_rate=args.sr,
                                                    norm="slaney", mel_scale="htk").numpy().astype(np.float64)
        got = specdist.mel_filterbank(args.sr, n_fft, n_mels)
        rel = np.abs(got - ref).max(axis=0) / ref.max(axis=0)
        support = int(np.sum((got > 0) != (ref > 0)))
        worst = max(worst, float(rel.max()))
        banks[(n_fft, n_mels)] = ref
        print(f"N {n_fft} n_mels {n_mels}: largest |difference| / filter peak {rel.max():.3e}; bins non-zero on one side only: {support}")
    rng = np.random.default_rng(0)
    n = 2 * args.sr
    t = np.arange(n) / args.sr
    x = 0.05 * rng.standard_normal(n) + 0.3 * np.sin(2 * np.pi * 440 * t) + 0.1 * np.sin(2 * np.pi * 9000 * t)
    x_hat = x + 0.02 * rng.standard_normal(n)
    mine, theirs = specdist.mel_distance(x_hat, x, args.sr), 0.0
    for (n_fft, n_mels), fb in banks.items():
        Mh, Mx = (np.abs(specdist.stft(x_hat, n_fft)) ** 2) @ fb, (np.abs(specdist.stft(x, n_fft)) ** 2) @ fb
        theirs += float(np.mean(np.abs(2 * np.log10(np.maximum(Mh, 1e-5)) - 2 * np.log10(np.maximum(Mx, 1e-5)))))
    print(f"mel distance of a seeded 2 s pair: this bank {mine:.12f}  torchaudio's bank {theirs:.12f}  diff {mine - theirs:+.3e}")
    print(f"pin_mel: largest |difference| / filter peak over the six banks = {worst:.3e} (torchaudio {getattr(torchaudio, '__version__', '?')})")
    return 0


if __name__ == "__main__":
    sys.exit(main())
