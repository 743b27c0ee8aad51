"""Segmental-SNR timing: segsnr.segsnr_batch (csrc/segsnr.hip) against the host yardstick segsnr.segsnr_detail one triple at a time, and
eval_cli's scoring with and without --ssnr, on the 64-file corpus of 1-4 s clips of scripts/cli_corpus_rtf.py (the seeded lengths and
signals of scripts/eval_timing.py and scripts/estoi_timing.py).  Loading is excluded everywhere: the signals are in host memory before a
clock starts.

  gpu            segsnr_batch as eval_cli calls it: rows built on the host, copied to the device, scored, read back
  gpu_resident   the same native calls on rows staged on the device beforehand (no host-to-device copy inside the clock)
  host           segsnr.segsnr_detail, float64 NumPy, one triple at a time in this process (both metrics from one call)
  score4/score6  eval_cli.score with the GPU scorer without / with ssnr=True

The sides run interleaved in one process, `--repeats` times each after one warm-up; medians are reported with every sample, and one box
calibration line (flowdec_amd.boxprobe.calibrate) says which box it was.  A report: nothing rests on these numbers.

    python scripts/segsnr_timing.py [--files 64] [--min-s 1] [--max-s 4] [--batch-files 8] [--repeats 5] [--out profiles/segsnr_timing.json]
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "segsnr_timing.json"))
    args = ap.parse_args()
    from flowdec_amd import _lib as L, boxprobe, eval_cli, metrics, segsnr
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
    plan = segsnr.segsnr_plan(sr)

    def clock(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    # the batches of segsnr_batch, staged on the device once
    staged = []
    for idx in metrics.length_sorted_batches([int(n) for n in lens], args.batch_files):
        B, Lmax = len(idx), max(int(lens[i]) for i in idx)
        (h, _), (x, ln) = (padded_rows([torch.as_tensor(l[i]).reshape(-1) for i in idx], Lmax, "cuda") for l in (hs, xs))
        nws = lib.fd_metrics_segsnr_workspace_bytes(plan.handle, B, Lmax)
        staged.append((idx, h, x, ln, torch.empty(nws, dtype=torch.uint8, device="cuda"), torch.empty(B, 2, dtype=torch.float64, device="cuda")))

    def resident():
        out = np.zeros((args.files, 2))
        for idx, h, x, ln, ws, val in staged:
            B, Lmax = x.shape
            L.check(lib.fd_metrics_segsnr(plan.handle, L.ptr(h), L.ptr(x), L.ptr(ln), B, Lmax, L.ptr(val), None, L.ptr(ws), ws.numel(), L.stream()))
            out[idx] = val.cpu().numpy()
        return out

    def host():
        details = [segsnr.segsnr_detail(h, x, sr) for h, x in zip(hs, xs)]
        return np.array([(d["fwssnr"], d["ssnr"]) for d in details])

    sides = {
        "gpu": lambda: segsnr.segsnr_batch(hs, xs, sr=sr, batch=args.batch_files),
        "gpu_resident": resident,
        "host": host,
        "score4": lambda: eval_cli.score(signals, sr, args.batch_files, eval_cli.GPU_SCORER),
        "score6": lambda: eval_cli.score(signals, sr, args.batch_files, eval_cli.GPU_SCORER, ssnr=True),
    }
    segsnr.critical_band_bank(sr, plan.n_fft)                     # the host bank is built once per process: outside the clock
    for name in ("gpu", "gpu_resident", "score4", "score6"):       # warm-up: plans, allocator
        sides[name]()
    times, values = {k: [] for k in sides}, {}
    for _ in range(args.repeats):
        for name, fn in sides.items():
            t, values[name] = clock(fn)
            times[name].append(t)
    med = {k: statistics.median(v) for k, v in times.items()}
    diff = np.abs(values["gpu"] - values["host"])
    out = {
        "what": "fwSSNR and SSNR of %d triples at 48 kHz (%.1f s of audio per signal), loading excluded" % (args.files, audio),
        "device": torch.cuda.get_device_name(0), "files": int(args.files), "audio_seconds": audio, "batch_files": args.batch_files, "repeats": args.repeats,
        "seconds": times, "median_s": med, "min_s": {k: min(v) for k, v in times.items()},
        "triples_per_second": {k: args.files / med[k] for k in ("gpu", "gpu_resident", "host")},
        "ratio_host_over_gpu": med["host"] / med["gpu"], "ratio_host_over_gpu_resident": med["host"] / med["gpu_resident"],
        "ssnr_added_to_score_s": med["score6"] - med["score4"], "score6_over_score4": med["score6"] / med["score4"],
        "max_abs_gpu_minus_host_db": {"fwSSNR": float(diff[:, 0].max()), "SSNR": float(diff[:, 1].max())},
        "gpu_equals_resident_bits": bool(values["gpu"].tobytes() == values["gpu_resident"].tobytes()),
        "gpu_equals_score6_bits": bool(values["gpu"].tobytes() == np.ascontiguousarray(values["score6"][:, 4:]).tobytes()),
        "score4_equals_score6_bits": bool(np.ascontiguousarray(values["score6"][:, :4]).tobytes() == values["score4"].tobytes()),
        "box_calibration": boxprobe.calibrate(),
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
