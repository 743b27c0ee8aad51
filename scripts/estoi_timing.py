"""ESTOI timing: metrics.estoi_batch (csrc/stoi.hip) against the host function metrics.estoi one triple at a time, and eval_cli's scoring
with and without --estoi, on the 64-file corpus of 1-4 s clips of scripts/cli_corpus_rtf.py (the seeded lengths and signals of
scripts/eval_timing.py).  Loading is excluded everywhere: the signals are in host memory before a clock starts.

  gpu            estoi_batch as eval_cli calls it: rows built on the host, copied to the device, scored, read back
  gpu_resident   the same native calls on rows staged on the device beforehand (no host-to-device copy inside the clock)
  host           metrics.estoi, float64 NumPy, one triple at a time in this process
  score4/score5  eval_cli.score with the GPU scorer without / with estoi=True

The sides run interleaved in one process, `--repeats` times each after one warm-up; medians are reported with every sample, and one box
calibration line (flowdec_amd.boxprobe.calibrate) says which box it was.  `--enhance-xrt` is the real-time factor of the enhancement the
scores belong to (MEASUREMENTS.md: the ragged corpus run), from which the share that ESTOI adds to an `enhance_cli --eval` run is formed.

    python scripts/estoi_timing.py [--files 64] [--min-s 1] [--max-s 4] [--batch-files 8] [--repeats 5] [--enhance-xrt 115]
                                   [--out profiles/estoi_timing.json]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=64)
    ap.add_argument("--min-s", type=float, default=1.0)
    ap.add_argument("--max-s", type=float, default=4.0)
    ap.add_argument("--batch-files", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--enhance-xrt", type=float, default=115.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "estoi_timing.json"))
    args = ap.parse_args()
    from flowdec_amd import _lib as L, boxprobe, eval_cli, metrics
    from flowdec_amd.batching import padded_rows

    sr = 48000
    rng = np.random.default_rng(0)
    lens = rng.integers(int(args.min_s * sr), int(args.max_s * sr) + 1, size=args.files)
    signals = []
    for n in lens:
        y = (0.1 * rng.standard_normal(int(n))).astype(np.float32)
        x = (y + 0.05 * rng.standard_normal(int(n))).astype(np.float32)
        h = (x + 0.02 * rng.standard_normal(int(n))).astype(np.float32)
        signals.append((torch.from_numpy(h), torch.from_numpy(x), torch.from_numpy(y)))
    hs, xs = [s[0] for s in signals], [s[1] for s in signals]
    audio = float(lens.sum()) / sr
    lib = L.load()
    plans = metrics.estoi_plans(sr)

    def clock(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    # the batches of estoi_batch, staged on the device once
    staged = []
    for idx in metrics.length_sorted_batches([int(n) for n in lens], args.batch_files):
        B, Lmax = len(idx), max(int(lens[i]) for i in idx)
        (h, _), (x, ln) = (padded_rows([torch.as_tensor(l[i]).reshape(-1) for i in idx], Lmax, "cuda") for l in (hs, xs))
        nws = lib.fd_metrics_estoi_workspace_bytes(B, Lmax, plans.o, plans.n)
        staged.append((idx, h, x, ln, torch.empty(nws, dtype=torch.uint8, device="cuda"), torch.empty(B, dtype=torch.float64, device="cuda"),
                       torch.empty(B, 3, dtype=torch.int32, device="cuda")))

    def resident():
        out = np.zeros(args.files)
        for idx, h, x, ln, ws, val, fr in staged:
            B, Lmax = x.shape
            L.check(lib.fd_metrics_estoi(plans.estoi, plans.resample, L.ptr(h), L.ptr(x), L.ptr(ln), B, Lmax, L.ptr(val), L.ptr(fr), L.ptr(ws), ws.numel(),
                                         L.stream()))
            out[idx] = val.cpu().numpy()
        return out

    sides = {
        "gpu": lambda: metrics.estoi_batch(hs, xs, sr=sr, batch=args.batch_files),
        "gpu_resident": resident,
        "host": lambda: np.array([metrics.estoi(h, x, sr) for h, x in zip(hs, xs)]),
        "score4": lambda: eval_cli.score(signals, sr, args.batch_files, eval_cli.GPU_SCORER),
        "score5": lambda: eval_cli.score(signals, sr, args.batch_files, eval_cli.GPU_SCORER, estoi=True),
    }
    for name in ("gpu", "gpu_resident", "score4", "score5"):       # warm-up: plans, allocator
        sides[name]()
    times, values = {k: [] for k in sides}, {}
    for _ in range(args.repeats):
        for name, fn in sides.items():
            t, values[name] = clock(fn)
            times[name].append(t)
    med = {k: statistics.median(v) for k, v in times.items()}
    enhance_s = audio / args.enhance_xrt
    out = {
        "what": "ESTOI of %d triples at 48 kHz (%.1f s of audio per signal), loading excluded" % (args.files, audio),
        "device": torch.cuda.get_device_name(0), "files": int(args.files), "audio_seconds": audio, "batch_files": args.batch_files, "repeats": args.repeats,
        "seconds": times, "median_s": med, "min_s": {k: min(v) for k, v in times.items()},
        "triples_per_second": {k: args.files / med[k] for k in ("gpu", "gpu_resident", "host")},
        "ratio_host_over_gpu": med["host"] / med["gpu"], "ratio_host_over_gpu_resident": med["host"] / med["gpu_resident"],
        "estoi_added_to_score_s": med["score5"] - med["score4"], "score5_over_score4": med["score5"] / med["score4"],
        "enhance_xrt_assumed": args.enhance_xrt, "enhance_seconds_at_that_rate": enhance_s,
        "estoi_share_of_enhance_eval_run": (med["score5"] - med["score4"]) / (enhance_s + med["score5"]),
        "host_estoi_over_enhance_seconds": med["host"] / enhance_s,
        "max_abs_gpu_minus_host": float(np.abs(values["gpu"] - values["host"]).max()),
        "gpu_equals_resident_bits": bool(values["gpu"].tobytes() == values["gpu_resident"].tobytes()),
        "gpu_equals_score5_bits": bool(values["gpu"].tobytes() == np.ascontiguousarray(values["score5"][:, 4]).tobytes()),
        "score4_equals_score5_bits": bool(np.ascontiguousarray(values["score5"][:, :4]).tobytes() == values["score4"].tobytes()),
        "box_calibration": boxprobe.calibrate(),
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
