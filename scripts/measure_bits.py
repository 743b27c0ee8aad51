"""One SHA-256 per case over the raw bytes of what the measurement entry points return on seeded float32 noise: run it against two
builds of the library (FLOWDEC_HIP_LIB=... selects one) and compare the listings line for line.  A refactor of the measurement kernels
must not change a line.  Every case runs twice, each clip alone (batch 1) and all clips in one batch.

    python scripts/measure_bits.py > new.txt
    FLOWDEC_HIP_LIB=/path/to/other/libflowdec_hip.so python scripts/measure_bits.py > old.txt

The shapes are the smallest at which each shared reduction can go wrong: SI-SxR slices that are empty, shorter than a wave, and longer
than one trip of the 256 threads (32769 samples in 128 slices); 8 and 9 frames around the log-spectral tile of 8; every window length
128 .. 4096 (every threads-per-frame geometry) and more than 256 frames for the finalise loops; one frame and 257 frames of the
segmental SNRs at three transform lengths."""
import hashlib
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def noise(lengths, seed, scale=0.1):
    torch.manual_seed(seed)
    return [scale * torch.randn(n, dtype=torch.float32) for n in lengths]


def digest(arrays) -> str:
    h = hashlib.sha256()
    for a in arrays:
        a = np.ascontiguousarray(a)
        h.update(str((a.dtype.str, a.shape)).encode())
        h.update(a.tobytes())
    return h.hexdigest()


def flat(out):
    """The arrays of one result: an array, a tuple of arrays, lists of per-clip arrays."""
    if isinstance(out, (tuple, list)):
        return [a for o in out for a in flat(o)]
    return [np.asarray(out)]


def main():
    from flowdec_amd import _lib as L, align, loudness, metrics, segsnr, specdist
    cases = []

    def case(name, n, fn):
        """fn(batch) -> result; listed for batch 1 and for one batch of all n clips"""
        for tag, batch in (("alone", 1), ("batch", n)):
            cases.append((f"{name} {tag}", digest(flat(fn(batch)))))

    lens = [1, 127, 129, 255, 32769]
    h, x, y = noise(lens, 1), noise(lens, 2), noise(lens, 3)
    case("sisxr", len(lens), lambda b: metrics.si_sxr_sums_batch(h, x, y, batch=b))
    lens = [257, 896, 1024]
    h, x = noise(lens, 4), noise(lens, 5)
    case("logspec 16k", len(lens), lambda b: metrics.logspec_mse_batch(h, x, sr=16000, batch=b))
    lens = [2049, 4100, 8200]
    hs, xs = noise(lens, 6), noise(lens, 7)
    case("specdist 48k", len(lens), lambda b: specdist.spectral_distances_batch(hs, xs, sr=48000, batch=b, return_terms=True))
    for sr in (8000, 16000, 48000):
        win, skip, _ = segsnr.frame_params(sr)
        lens = [win + skip, win + 257 * skip]
        hg, xg = noise(lens, 8 + sr), noise(lens, 9 + sr)
        case(f"segsnr {sr}", len(lens), lambda b: segsnr.segsnr_batch(hg, xg, sr=sr, batch=b, return_frames=True))
    lens = [4400, 20000]
    he, xe = noise(lens, 10), noise(lens, 11)
    xe = [a + 0.5 * b for a, b in zip(xe, he)]                     # correlated, as an estimate and its target are
    for sr in (10000, 16000):
        case(f"estoi {sr}", len(lens), lambda b: metrics.estoi_batch(he, xe, sr=sr, batch=b, return_frames=True))
    pairs = [(1, 5), (300, 257), (5000, 4000)]
    a_, b_ = noise([p for p, _ in pairs], 12), noise([q for _, q in pairs], 13)
    for M in (1, 200):
        case(f"lags M{M}", len(pairs), lambda b: align.lags_batch(a_, b_, M, batch=b, return_xcorr=True))
        for pol in (False, True):
            case(f"lags_frac M{M} polarity {int(pol)}", len(pairs), lambda b: align.lags_batch_frac(a_, b_, M, 64, 32, pol, batch=b, return_xcorr=True))
    lens = [4799, 19200, 48000]
    sl = noise(lens, 14)
    case("loudness 48k", len(lens), lambda b: loudness.loudness_batch(sl, sr=48000, batch=b, return_counts=True))
    case("loudness_ms 48k", len(lens), lambda b: loudness.loudness_ms_batch(sl, sr=48000, batch=b))

    print(f"# {len(cases)} cases, library {os.path.basename(os.path.dirname(L.LIB_PATH))}/{os.path.basename(L.LIB_PATH)}", file=sys.stderr)
    for name, d in cases:
        print(f"{name}: {d}")


if __name__ == "__main__":
    main()
