#!/usr/bin/env python
"""Integrated loudness: timing (MEASUREMENTS.md "Loudness").  Nothing is asserted except that the routes agree.

Two corpora of seeded noise under a slow envelope, in memory, float32 at 48 kHz: 24 clips of 30 s, and one clip of 10 minutes.  Routes,
interleaved in one process, medians over --repeats:

  gpu_total      loudness.loudness_batch on host clips: staging (zero-padded rows, one host-to-device copy per batch) + kernels + read-back
  gpu_resident   the same call on clips that already live on the device (what eval_cli --resample device leaves)
  gpu_kernels    fd_loudness alone on rows staged beforehand, between two events on the stream: loading reported apart
  yardstick      loudness.integrated_loudness, the NumPy float64 definition the kernels follow bit for bit
  scipy          scipy.signal.lfilter twice + NumPy block sums and gates (tests/loudness_cases.py reference_reading)

    python scripts/loudness_timing.py [--clips 24] [--seconds 30] [--long-seconds 600] [--batch 8] [--repeats 5] [--out profiles/loudness_timing.json]
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
sys.path.insert(0, os.path.join(ROOT, "tests"))


def corpus(n, seconds, seed):
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        L = int(seconds * 48000) - 997 * k
        t = np.arange(L) / 48000.0
        env = 0.05 + 0.1 * (1.0 + np.sin(2 * np.pi * t / (7.0 + k)))
        out.append((env * rng.standard_normal(L)).astype(np.float32))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=24)
    ap.add_argument("--seconds", type=float, default=30.0)
    ap.add_argument("--long-seconds", type=float, default=600.0)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "loudness_timing.json"))
    args = ap.parse_args()
    from flowdec_amd import _lib as L
    from flowdec_amd import boxprobe, loudness
    from flowdec_amd.batching import length_sorted_batches, padded_rows
    from loudness_cases import reference_reading
    lib = L.load()

    def clock(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    def kernels_only(clips):
        """fd_loudness on rows staged beforehand -> (seconds between two stream events, ms)."""
        lens = [len(c) for c in clips]
        staged = []
        for idx in length_sorted_batches(lens, args.batch):
            Lmax = max(lens[i] for i in idx)
            rows, ln = padded_rows([torch.from_numpy(clips[i]) for i in idx], Lmax, "cuda")
            nws = lib.fd_loudness_workspace_bytes(len(idx), Lmax)
            staged.append((idx, rows, ln, Lmax, torch.empty(nws, dtype=torch.uint8, device="cuda"), nws,
                           torch.empty(len(idx), dtype=torch.float64, device="cuda"), torch.empty(len(idx), 3, dtype=torch.int32, device="cuda")))
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for idx, rows, ln, Lmax, ws, nws, ms, counts in staged:
            L.check(lib.fd_loudness(L.ptr(rows), L.ptr(ln), len(idx), Lmax, L.ptr(ms), L.ptr(counts), L.ptr(ws), nws, L.stream()))
        b.record()
        torch.cuda.synchronize()
        out = np.zeros(len(clips))
        for idx, *_, ms, _ in staged:
            out[idx] = ms.cpu().numpy()
        return a.elapsed_time(b) / 1e3, loudness.lufs_of(out)

    res = {"device": torch.cuda.get_device_name(0), "batch": args.batch, "repeats": args.repeats, "chunk_samples": loudness.CHUNK, "corpora": {}}
    for name, clips in (("%d clips of %g s" % (args.clips, args.seconds), corpus(args.clips, args.seconds, 0)),
                        ("1 clip of %g s" % args.long_seconds, corpus(1, args.long_seconds, 1))):
        resident = [torch.from_numpy(c).cuda() for c in clips]
        routes = {"gpu_total": lambda: loudness.loudness_batch(clips, batch=args.batch),
                  "gpu_resident": lambda: loudness.loudness_batch(resident, batch=args.batch),
                  "yardstick": lambda: np.array([loudness.integrated_loudness(c) for c in clips]),
                  "scipy": lambda: np.array([reference_reading(c, loudness.K48, loudness.ABS_GATE)[0] for c in clips])}
        routes["gpu_total"](), kernels_only(clips)                       # warm-up: code objects, allocator
        times = {k: [] for k in list(routes) + ["gpu_kernels"]}
        got = {}
        for r in range(args.repeats):
            for k, fn in routes.items():
                if k in ("yardstick", "scipy") and r >= 2:
                    continue
                t, got[k] = clock(fn)
                times[k].append(t)
            t, got["gpu_kernels"] = kernels_only(clips)
            times["gpu_kernels"].append(t)
        med = {k: statistics.median(v) for k, v in times.items()}
        audio_s = sum(len(c) for c in clips) / 48000.0
        same = lambda a, b: bool(np.array_equal(np.asarray(a).view(np.uint64), np.asarray(b).view(np.uint64)))
        res["corpora"][name] = {"audio_seconds": audio_s, "seconds": times, "median_s": med, "audio_seconds_per_second": {k: audio_s / v for k, v in med.items()},
                                "gpu_equals_yardstick_bits": same(got["gpu_total"], got["yardstick"]) and same(got["gpu_resident"], got["yardstick"])
                                and same(got["gpu_kernels"], got["yardstick"]),
                                "max_abs_yardstick_minus_scipy_db": float(np.max(np.abs(got["yardstick"] - got["scipy"]))),
                                "lufs_first": float(got["gpu_total"][0])}
        print(json.dumps({name: res["corpora"][name]["median_s"], "bits": res["corpora"][name]["gpu_equals_yardstick_bits"]}), flush=True)
        assert res["corpora"][name]["gpu_equals_yardstick_bits"], "the GPU and the yardstick disagree"
    res["box_calibration"] = boxprobe.calibrate()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
