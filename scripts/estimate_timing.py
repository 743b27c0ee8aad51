"""Parameter-estimation timing: flowdec_amd.estimate.estimate_params on the GPU against a host computation of the same statistics
(torch-CPU stft, the compression, every bin concatenated, np.quantile -- this project's restatement of what the reference's
scripts/estimate_flowdec_params.py computes, not the reference), on `--pairs` synthetic pairs of `--seconds` s at 48 kHz.

Loading and computing are reported separately: the pairs are first written as PCM16 wavs into a temporary directory and read back with
audio.load_mono (what estimate_cli does per file), then both sides compute from the clips in host memory.  The GPU side includes its
host-to-device copies and the read-back.  The two sides run interleaved, `--repeats` times each after one warm-up of the GPU side.

    python scripts/estimate_timing.py [--pairs 256] [--seconds 2] [--batch-pairs 64] [--repeats 3] [--out profiles/estimate_timing.json]
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time
import wave

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ALPHA, NFFT, HOP, Q = 0.3, 1534, 384, 0.997


def host_estimate(xs, ys, per_band):
    """The script's statistics on the host, float32: -> (q(|X_c|), max |X_c|, quantile of the RMSEs)."""
    win = torch.signal.windows.hann(NFFT)

    def feats(a):
        X = torch.stft(a, NFFT, hop_length=HOP, window=win, center=True, onesided=True, return_complex=True)
        return X.abs() ** ALPHA * torch.exp(1j * X.angle())
    fx, fy = [], []
    for x, y in zip(xs, ys):
        nf = y.abs().max() + 1e-5
        fx.append(feats(x / nf)); fy.append(feats(y / nf))
    bins = torch.cat([f.reshape(-1) for f in fx]).abs().numpy()
    q_x = np.quantile(bins, Q)
    F = fx[0].shape[-2]
    if per_band:
        rm = np.array([torch.linalg.norm(b - a, ord=2, dim=-1).numpy() / F ** 0.5 for a, b in zip(fx, fy)])
        return q_x, bins.max(), np.quantile(rm, Q, axis=0)
    rm = np.array([torch.linalg.norm((b - a).reshape(-1), ord=2).item() / a.numel() ** 0.5 for a, b in zip(fx, fy)])
    return q_x, bins.max(), np.quantile(rm, Q)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=256)
    ap.add_argument("--seconds", type=float, default=2.0)
    ap.add_argument("--batch-pairs", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--per-band", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "estimate_timing.json"))
    args = ap.parse_args()
    from flowdec_amd import estimate as E
    from flowdec_amd.audio import load_mono

    n = int(args.seconds * 48000)
    rng = np.random.default_rng(0)
    with tempfile.TemporaryDirectory() as d:
        paths = []
        for i in range(args.pairs):
            x = np.clip(3000 * rng.standard_normal(n), -32768, 32767).astype("<i2")
            y = np.clip(x + 300 * rng.standard_normal(n), -32768, 32767).astype("<i2")
            for tag, s in (("x", x), ("y", y)):
                p = os.path.join(d, f"{tag}{i}.wav")
                with wave.open(p, "wb") as w:
                    w.setnchannels(1); w.setsampwidth(2); w.setframerate(48000); w.writeframes(s.tobytes())
                paths.append(p)
        t0 = time.perf_counter()
        clips = [load_mono(p, 48000) for p in paths]
        load_s = time.perf_counter() - t0
    xs, ys = clips[0::2], clips[1::2]

    def gpu():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = E.estimate_params(xs, ys, alpha=ALPHA, n_fft=NFFT, hop=HOP, qx=Q, qrmse=Q, per_band=args.per_band, batch_pairs=args.batch_pairs)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, r

    def host():
        t0 = time.perf_counter()
        r = host_estimate(xs, ys, args.per_band)
        return time.perf_counter() - t0, r

    gpu()          # warm-up: the transform plan, the allocator
    host_s, gpu_s = [], []
    for _ in range(args.repeats):
        t, hv = host(); host_s.append(t)
        t, gv = gpu(); gpu_s.append(t)
    hm, gm = statistics.median(host_s), statistics.median(gpu_s)
    out = {
        "what": "beta / sigma_y statistics of %d pairs of %.1f s (%d bins per side), loading reported apart" % (args.pairs, args.seconds, gv.n_bins),
        "device": torch.cuda.get_device_name(0), "pairs": args.pairs, "seconds": args.seconds, "per_band": bool(args.per_band),
        "batch_pairs": args.batch_pairs, "host_threads": torch.get_num_threads(), "repeats": args.repeats,
        "load_seconds": load_s, "load_ms_per_file": 1e3 * load_s / len(paths),
        "host_seconds": host_s, "gpu_seconds": gpu_s, "host_median_s": hm, "gpu_median_s": gm, "ratio_host_over_gpu": hm / gm,
        "rel_diff_abs_quantile_x": float(abs(gv.abs_quantile_x - hv[0]) / hv[0]), "rel_diff_max_abs_x": float(abs(gv.max_abs_x - hv[1]) / hv[1]),
        "max_rel_diff_rmse_quantile": float(np.max(np.abs(np.asarray(gv.rmse_quantile) - hv[2]) / hv[2])),
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
