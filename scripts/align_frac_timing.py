#!/usr/bin/env python
"""Sub-sample alignment: timing and the estimate demonstration (MEASUREMENTS.md "Sub-sample alignment").

Timing, on the 64-clip corpus of scripts/align_timing.py (1-4 s at 48 kHz, seeded) as (clean, coded) pairs in memory: coded = clean read
a seeded -40 .. +40 ms plus a seeded fraction of a sample EARLIER through align.frac_shift (so it is late by that much), every fourth
one inverted, plus 2 % noise.  For a search of +-100 ms (M = 4800), in pairs per second, the three routes interleaved in one process:

  integer        the parent's path: align.lags_batch, then the views of align.align_triple's cut (no kernel)
  fractional     align.lags_batch_frac (correlation + finalise on |c| + refinement), then align.cut_frac with align.shift_batch
  host           the yardstick pair align.host_lags_frac + align.host_shift on the first --yardstick-pairs pairs

Estimate demonstration: estimate.estimate_params(per_band=True) on pairs whose ONLY defect is a delay of 2.5 samples (white noise, coded
= clean read 2.5 samples earlier): unaligned, integer-aligned and fractionally aligned, sigma_y at a low, a middle and the top band, beside
2 sin(omega tau / 2) for tau = 2.5 (unaligned) and tau = 0.5 (what a whole-sample alignment leaves).  Nothing is asserted.

    python scripts/align_frac_timing.py [--files 64] [--batch 8] [--repeats 5] [--out profiles/align_frac_timing.json]
"""
import argparse
import json
import math
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
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--yardstick-pairs", type=int, default=2)
    ap.add_argument("--estimate-pairs", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "align_frac_timing.json"))
    args = ap.parse_args()
    from flowdec_amd import align, boxprobe, estimate

    sr, Q, W, M = 48000, align.FRAC_Q, align.FRAC_W, 4800
    rng = np.random.default_rng(0)
    lens = rng.integers(int(args.min_s * sr), int(args.max_s * sr) + 1, size=args.files)
    clean = [(0.1 * rng.standard_normal(int(n))).astype(np.float32) for n in lens]
    true_q = rng.integers(-1920, 1921, size=args.files) * Q + rng.integers(0, Q, size=args.files)
    true_s = np.where(np.arange(args.files) % 4 == 3, -1, 1)
    coded = [align.frac_shift(x, -int(l), int(g), Q, W, 0, len(x)) + (0.002 * rng.standard_normal(len(x))).astype(np.float32)
             for x, l, g in zip(clean, true_q, true_s)]
    xs, ys = [torch.from_numpy(x) for x in clean], [torch.from_numpy(y) for y in coded]

    null = open(os.devnull, "w")                                       # the warnings and summary lines of align_pairs

    def clock(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    def integer():
        lags = align.lags_batch(xs, ys, M, batch=args.batch)
        return lags, [align.align_triple(y, x, y, int(l), int(l))[:2] for x, y, l in zip(xs, ys, lags)]

    def fractional():
        return align.align_pairs(xs, ys, M, True, True, Q, W, args.batch, err=null)

    k = min(args.yardstick_pairs, args.files)

    def host():
        return align.align_pairs(xs[:k], ys[:k], M, True, True, Q, W, args.batch, None, align.host_lags, align.host_lags_frac, align.host_shift,
                                 err=null)

    integer(), fractional()                                            # warm-up: code objects, allocator
    times = {"integer": [], "fractional": [], "host": []}
    got = {}
    for r in range(args.repeats):
        for name, fn in (("integer", integer), ("fractional", fractional), ("host", host)):
            if name == "host" and r >= 1:
                continue
            t, got[name] = clock(fn)
            times[name].append(t)
    med = {name: statistics.median(v) for name, v in times.items()}
    lag_q, sign = got["fractional"][2], got["fractional"][3]
    res = {"what": "%d (clean, coded) pairs at 48 kHz, %.1f s of audio per signal, search +-100 ms (M = %d), Q = %d, W = %d" % (args.files, float(lens.sum()) / sr, M, Q, W),
           "device": torch.cuda.get_device_name(0), "batch": args.batch, "repeats": args.repeats, "seconds": times, "median_s": med,
           "pairs_per_second": {"integer": args.files / med["integer"], "fractional": args.files / med["fractional"], "host": k / med["host"]},
           "yardstick_pairs": k,
           "fractional_within_one_grid_step_of_true": int(np.sum(np.abs(lag_q - true_q) <= 1)), "fractional_max_error_in_grid_steps": int(np.abs(lag_q - true_q).max()),
           "signs_right": int(np.sum(sign == true_s)), "integer_lag_equals_rounded_true": int(np.sum(got["integer"][0] == np.round(true_q / Q))),
           "host_equals_gpu_lag_q": bool(np.array_equal(got["host"][2], lag_q[:k])),
           "host_equals_gpu_samples": bool(all(torch.equal(a, b) for a, b in zip(got["host"][1], got["fractional"][1][:k])))}
    print(json.dumps({"pairs_per_second": res["pairs_per_second"]}), flush=True)

    # ---- the estimate demonstration --------------------------------------------------------------------------------------------------------
    n_fft, hop, alpha, tau, L = 1534, 384, 0.3, 2.5, 2 * sr
    xs_e = [(0.1 * rng.standard_normal(L + 200)).astype(np.float32) for _ in range(args.estimate_pairs)]
    ys_e = [align.frac_shift(x, -int(tau * Q), 1, Q, W, 0, len(x)) for x in xs_e]
    tx, ty = [torch.from_numpy(x) for x in xs_e], [torch.from_numpy(y) for y in ys_e]
    runs = {"unaligned": (tx, ty), "integer": align.align_pairs(tx, ty, 480, False, False, Q, W, args.batch, err=null)[:2],
            "fractional": align.align_pairs(tx, ty, 480, True, False, Q, W, args.batch, err=null)[:2]}
    F = n_fft // 2 + 1
    bands = {"low": 8, "middle": F // 2, "top": F - 2}
    demo = {"pairs": args.estimate_pairs, "tau_samples": tau, "n_fft": n_fft, "hop": hop, "alpha": alpha, "bands": bands, "sigma_y": {}, "beta": {}}
    for name, (a, b) in runs.items():
        cut = [(x[100:100 + L], y[100:100 + L]) for x, y in zip(a, b)]       # one length for all three runs, away from the ends
        r = estimate.estimate_params([x for x, _ in cut], [y for _, y in cut], alpha=alpha, n_fft=n_fft, hop=hop, per_band=True, batch_pairs=args.batch)
        demo["sigma_y"][name] = {k: float(r.sigma_y[f]) for k, f in bands.items()}
        demo["beta"][name] = float(r.beta)
    demo["two_sin_omega_tau_half"] = {k: {"tau_2.5": 2 * abs(math.sin(math.pi * f / (F - 1) * 2.5 / 2)), "tau_0.5": 2 * abs(math.sin(math.pi * f / (F - 1) * 0.5 / 2))}
                                      for k, f in bands.items()}
    res["estimate_demo"] = demo
    res["box_calibration"] = boxprobe.calibrate()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
