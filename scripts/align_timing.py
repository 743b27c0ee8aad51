#!/usr/bin/env python
"""Alignment timing on the 64-file corpus of scripts/cli_corpus_rtf.py (1-4 s clips at 48 kHz, seeded) as a triples list on disk: x the
clean clip, x_hat = x delayed by a seeded lag within +-40 ms plus 2 % noise, y = x delayed by a seeded lag within +-5 ms plus 50 % noise.
For a search of +-100 ms (M = 4800) and of +-1 s (M = 48000), both lags of every triple (128 pairs), loading reported apart:

  gpu            flowdec_amd.align.lags_batch: rows built on the host, copied, correlated, the lags read back
  gpu_resident   the same native calls (fd_xcorr_lags) on rows already on the device, c = NULL
  scipy_fft      the host route a user has today: scipy.signal.correlate(b, a, mode="full", method="fft") per pair in float64, cut to
                 +-M, argmax
  (the float64 yardstick align.host_lags, a dot product per lag, is timed on the first --yardstick-pairs pairs only: it is the definition,
  not a route)

and eval_cli on the same list with and without --align 100 (wall time, loading included).  The calibration line
(flowdec_amd.boxprobe.calibrate) says which box it was.

    python scripts/align_timing.py [--files 64] [--batch-files 8] [--repeats 5] [--out profiles/align_timing.json]
"""
import argparse
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def delayed(x, d):
    out = np.zeros_like(x)
    if d >= 0:
        out[d:] = x[:len(x) - d]
    else:
        out[:d] = x[-d:]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=64)
    ap.add_argument("--min-s", type=float, default=1.0)
    ap.add_argument("--max-s", type=float, default=4.0)
    ap.add_argument("--batch-files", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--yardstick-pairs", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "align_timing.json"))
    args = ap.parse_args()
    from scipy.signal import correlate
    from flowdec_amd import _lib as L, align, audio, boxprobe, eval_cli
    from flowdec_amd.batching import length_sorted_batches, padded_rows

    sr = 48000
    lib = L.load()
    tmp = tempfile.mkdtemp(prefix="fd_align_")
    try:
        rng = np.random.default_rng(0)
        lens = rng.integers(int(args.min_s * sr), int(args.max_s * sr) + 1, size=args.files)
        clean = [(0.1 * rng.standard_normal(int(n))).astype(np.float32) for n in lens]
        true_h, true_y = rng.integers(-1920, 1921, size=args.files), rng.integers(-240, 241, size=args.files)
        lines = []
        for i, x in enumerate(clean):
            h = delayed(x, int(true_h[i])) + (0.002 * rng.standard_normal(len(x))).astype(np.float32)
            y = delayed(x, int(true_y[i])) + (0.05 * rng.standard_normal(len(x))).astype(np.float32)
            paths = [os.path.join(tmp, f"{k}{i:03d}.wav") for k in ("clean", "noisy", "enh")]
            for p, s in zip(paths, (x, y, h)):
                audio.save_wav(p, torch.from_numpy(s), sr)
            lines.append(" ---> ".join(paths))
        lst = os.path.join(tmp, "triples_list.txt")
        with open(lst, "w") as f:
            f.write("\n".join(lines) + "\n")
        audio_s = float(lens.sum()) / sr

        def clock(fn):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            return time.perf_counter() - t0, out

        def load():
            return [tuple(audio.load_mono(p, sr) for p in (t.x_hat, t.x, t.y)) for t in eval_cli.read_triples(lst)]

        t_load, sig = zip(*[clock(load) for _ in range(args.repeats)])
        sig = sig[-1]
        as_ = [x for _, x, _ in sig] * 2
        bs = [h for h, _, _ in sig] + [y for _, _, y in sig]
        want = np.concatenate([true_h, true_y]).astype(np.int64)
        n_pairs = len(as_)

        def scipy_route(M):
            def run():
                out = np.zeros(n_pairs, np.int64)
                for i, (a, b) in enumerate(zip(as_, bs)):
                    a64, b64 = a.numpy().astype(np.float64), b.numpy().astype(np.float64)
                    full = correlate(b64, a64, mode="full", method="fft")          # index k is lag k - (len(a) - 1)
                    l = np.arange(-M, M + 1)
                    k = l + len(a64) - 1
                    ok = (k >= 0) & (k < len(full))
                    c = np.where(ok, full[np.clip(k, 0, len(full) - 1)], 0.0)
                    out[i] = align.pick_lag(c)
                return out
            return run

        def resident_route(M):
            staged = []
            la, lb = [int(c.numel()) for c in as_], [int(c.numel()) for c in bs]
            for idx in length_sorted_batches([max(p, q) for p, q in zip(la, lb)], args.batch_files):
                B, La, Lb = len(idx), max(la[i] for i in idx), max(lb[i] for i in idx)
                ra, na = padded_rows([as_[i] for i in idx], La, "cuda")
                rb, nb = padded_rows([bs[i] for i in idx], Lb, "cuda")
                nws = lib.fd_xcorr_workspace_bytes(B, La, Lb, M)
                staged.append((idx, ra, rb, na, nb, torch.empty(nws, dtype=torch.uint8, device="cuda"), torch.empty(B, dtype=torch.int32, device="cuda")))

            def run():
                out = np.zeros(n_pairs, np.int64)
                for idx, ra, rb, na, nb, ws, lags in staged:
                    B, La, Lb = ra.shape[0], ra.shape[1], rb.shape[1]
                    L.check(lib.fd_xcorr_lags(L.ptr(ra), L.ptr(rb), L.ptr(na), L.ptr(nb), B, La, Lb, M, None, L.ptr(lags), L.ptr(ws), ws.numel(), L.stream()))
                    out[idx] = lags.cpu().numpy()
                return out
            return run

        res = {"what": "both lags of %d triples (%d pairs) at 48 kHz, %.1f s of audio per signal" % (args.files, n_pairs, audio_s),
               "device": torch.cuda.get_device_name(0), "files": int(args.files), "pairs": n_pairs, "audio_seconds": audio_s, "batch_files": args.batch_files,
               "repeats": args.repeats, "kernel_variant": "v_mfma_f64_16x16x4_f64 from LDS (2048 lags x 32768 samples per workgroup)",
               "load_seconds": {"all": list(t_load), "median": statistics.median(t_load)}, "search": {}}
        for ms, M in ((100, 4800), (1000, 48000)):
            sides = {"gpu": lambda M=M: align.lags_batch(as_, bs, M, batch=args.batch_files), "gpu_resident": resident_route(M), "scipy_fft": scipy_route(M)}
            sides["gpu"](), sides["gpu_resident"]()                        # warm-up: code objects, allocator
            times, values = {k: [] for k in sides}, {}
            for r in range(args.repeats):
                for name, fn in sides.items():
                    if name == "scipy_fft" and r >= 2:
                        continue
                    t, values[name] = clock(fn)
                    times[name].append(t)
            k = min(args.yardstick_pairs, n_pairs)
            t_yard, yard = clock(lambda: align.host_lags(as_[:k], bs[:k], M))
            med = {name: statistics.median(v) for name, v in times.items()}
            macs = float(sum((2 * M + 1) * min(int(a.numel()), int(b.numel())) for a, b in zip(as_, bs)))
            res["search"][f"{ms}_ms"] = {
                "max_lag": M, "seconds": times, "median_s": med, "ratio_scipy_over_gpu": med["scipy_fft"] / med["gpu"],
                "ratio_scipy_over_gpu_resident": med["scipy_fft"] / med["gpu_resident"], "float64_fma_upper_count": macs,
                "gpu_resident_tera_fma_per_second": macs / med["gpu_resident"] / 1e12,
                "yardstick_seconds_per_pair": t_yard / max(k, 1), "yardstick_pairs": k,
                "lags_equal_true": {name: int(np.sum(v == want)) for name, v in values.items()},
                "gpu_equals_resident": bool(np.array_equal(values["gpu"], values["gpu_resident"])),
                "gpu_equals_scipy": int(np.sum(values["gpu"] == values["scipy_fft"])), "gpu_equals_yardstick": bool(np.array_equal(values["gpu"][:k], yard))}
            print(json.dumps({f"{ms}_ms": res["search"][f"{ms}_ms"]["median_s"]}), flush=True)
        cli = {}
        for name, extra in (("plain", []), ("align_100ms", ["--align", "100"])):
            argv = ["--triples", lst, "--out", os.path.join(tmp, name + ".csv"), "--batch-files", str(args.batch_files)] + extra
            eval_cli.run(argv)                                             # warm-up: plans, allocator
            ts = [clock(lambda: eval_cli.run(argv))[0] for _ in range(args.repeats)]
            cli[name] = {"seconds": ts, "median_s": statistics.median(ts)}
        res["eval_cli_wall_seconds_incl_loading"] = cli
        res["eval_cli_align_minus_plain_s"] = cli["align_100ms"]["median_s"] - cli["plain"]["median_s"]
        res["box_calibration"] = boxprobe.calibrate()
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
        print(json.dumps(res))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
