#!/usr/bin/env python
"""Loudness report (integrated loudness, loudness range, true peak): timing (MEASUREMENTS.md "Loudness report").  Nothing is asserted
except that the routes agree.

Two corpora of seeded noise under a slow envelope, in memory, float32 at 48 kHz: 64 files of about 10 s, and one file of 10 minutes.
Routes, interleaved in one process, medians over --repeats (the host route runs once: it is the slow one):

  gpu_report     loudness.loudness_report_batch on host clips: ONE staging (zero-padded rows, one host-to-device copy per batch), the
                 energies once for the gate and for the range, the true peak on the same rows, read-back
  gpu_resident   the same call on clips that already live on the device
  gpu_three      loudness_batch + loudness_range_batch + true_peak_batch on the resident clips: three stagings, the energies twice
  gpu_peak       true_peak_batch alone on the resident clips
  gpu_range      loudness_range_batch alone on the resident clips
  yardsticks     integrated_loudness + loudness_range + true_peak of every clip: the NumPy float64 definitions the kernels follow bit for bit

    python scripts/loudness_report_timing.py [--clips 64] [--seconds 10] [--long-seconds 600] [--batch 8] [--repeats 5]
                                             [--out profiles/loudness_report_timing.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from loudness_timing import corpus  # noqa: E402  (the sibling script's corpus: seeded noise under a slow envelope)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=64)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--long-seconds", type=float, default=600.0)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "loudness_report_timing.json"))
    args = ap.parse_args()
    from flowdec_amd import boxprobe, loudness

    def clock(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    def three(clips):
        return {"lufs": loudness.loudness_batch(clips, batch=args.batch), "lra": loudness.loudness_range_batch(clips, batch=args.batch),
                "dbtp": loudness.true_peak_batch(clips, batch=args.batch)}

    def yardsticks(clips):
        return {"lufs": np.array([loudness.integrated_loudness(c) for c in clips]), "lra": np.array([loudness.loudness_range(c) for c in clips]),
                "dbtp": np.array([loudness.true_peak(c) for c in clips])}

    def same(a, b):
        return all(bool(np.array_equal(np.asarray(a[k], np.float64).view(np.uint64), np.asarray(b[k], np.float64).view(np.uint64))) for k in ("lufs", "lra", "dbtp"))

    res = {"device": torch.cuda.get_device_name(0), "batch": args.batch, "repeats": args.repeats, "true_peak_taps_per_phase": 2 * loudness.TP_W,
           "corpora": {}}
    for name, clips in (("%d clips of %g s" % (args.clips, args.seconds), corpus(args.clips, args.seconds, 0)),
                        ("1 clip of %g s" % args.long_seconds, corpus(1, args.long_seconds, 1))):
        resident = [torch.from_numpy(c).cuda() for c in clips]
        routes = {"gpu_report": lambda: loudness.loudness_report_batch(clips, batch=args.batch),
                  "gpu_resident": lambda: loudness.loudness_report_batch(resident, batch=args.batch),
                  "gpu_three": lambda: three(resident),
                  "gpu_peak": lambda: loudness.true_peak_batch(resident, batch=args.batch),
                  "gpu_range": lambda: loudness.loudness_range_batch(resident, batch=args.batch),
                  "yardsticks": lambda: yardsticks(clips)}
        routes["gpu_report"](), routes["gpu_three"]()                     # warm-up: code objects, allocator, the tap table
        times, got = {k: [] for k in routes}, {}
        for r in range(args.repeats):
            for k, fn in routes.items():
                if k == "yardsticks" and r >= 1:
                    continue
                t, got[k] = clock(fn)
                times[k].append(t)
        med = {k: statistics.median(v) for k, v in times.items()}
        audio_s = sum(len(c) for c in clips) / 48000.0
        bits = same(got["gpu_report"], got["yardsticks"]) and same(got["gpu_resident"], got["yardsticks"]) and same(got["gpu_three"], got["yardsticks"])
        res["corpora"][name] = {"audio_seconds": audio_s, "seconds": times, "median_s": med, "audio_seconds_per_second": {k: audio_s / v for k, v in med.items()},
                                "gpu_equals_yardsticks_bits": bits, "first": {k: float(got["gpu_report"][k][0]) for k in ("lufs", "lra", "dbtp")}}
        print(json.dumps({name: med, "bits": bits}), flush=True)
        assert bits, "the GPU and the yardsticks disagree"
    res["box_calibration"] = boxprobe.calibrate()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
