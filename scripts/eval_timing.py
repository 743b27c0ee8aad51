"""Evaluation timing: the host functions of flowdec_amd/metrics.py, one triple at a time in one process, against eval_cli's GPU batches
(metrics.si_sxr_batch + metrics.logspec_mse_batch), on the 64-file corpus of 1-4 s clips of scripts/cli_corpus_rtf.py (the same seeded
lengths and noise as its inputs; the "enhanced" and "clean" signals are seeded perturbations of them -- the metrics' cost does not depend
on the values).  Loading is excluded from both sides: the signals are in host memory before the clock starts; the GPU side includes its
host-to-device copies and the read-back.  The two sides run interleaved in one call, `--repeats` times each after one warm-up.

    python scripts/eval_timing.py [--files 64] [--min-s 1] [--max-s 4] [--batch-files 8] [--repeats 3] [--out profiles/eval_timing.json]
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
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eval_timing.json"))
    args = ap.parse_args()
    from flowdec_amd import eval_cli

    rng = np.random.default_rng(0)
    lens = rng.integers(int(args.min_s * 48000), int(args.max_s * 48000) + 1, size=args.files)
    signals = []
    for n in lens:
        y = (0.1 * rng.standard_normal(int(n))).astype(np.float32)       # cli_corpus_rtf.py's input files
        x = (y + 0.05 * rng.standard_normal(int(n))).astype(np.float32)
        h = (x + 0.02 * rng.standard_normal(int(n))).astype(np.float32)
        signals.append((torch.from_numpy(h), torch.from_numpy(x), torch.from_numpy(y)))
    audio = float(lens.sum()) / 48000

    def timed(scorer):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        values = eval_cli.score(signals, 48000, args.batch_files, scorer)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, values

    timed(eval_cli.GPU_SCORER)            # warm-up: the transform plan, the allocator
    host_s, gpu_s = [], []
    for _ in range(args.repeats):
        t, host_values = timed(eval_cli.HOST_SCORER)
        host_s.append(t)
        t, gpu_values = timed(eval_cli.GPU_SCORER)
        gpu_s.append(t)
    host, gpu = statistics.median(host_s), statistics.median(gpu_s)
    out = {
        "what": "SI-SDR/SI-SIR/SI-SAR + LogSpecMSE of %d triples (%.1f s of audio per signal), loading excluded" % (args.files, audio),
        "device": torch.cuda.get_device_name(0), "files": int(args.files), "audio_seconds": audio, "batch_files": args.batch_files,
        "repeats": args.repeats, "host_seconds": host_s, "gpu_seconds": gpu_s, "host_median_s": host, "gpu_median_s": gpu,
        "ratio_host_over_gpu": host / gpu,
        "host_ms_per_triple": 1e3 * host / args.files, "gpu_ms_per_triple": 1e3 * gpu / args.files,
        "max_abs_sisxr_diff_db": float(np.abs(host_values[:, :3] - gpu_values[:, :3]).max()),
        "max_rel_logspec_diff": float((np.abs(host_values[:, 3] - gpu_values[:, 3]) / host_values[:, 3]).max()),
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
