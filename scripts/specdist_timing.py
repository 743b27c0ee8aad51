"""Spectral-distance timing on the 64-file corpus of scripts/eval_timing.py (1-4 s clips at 48 kHz, seeded; loading excluded everywhere):

  host        flowdec_amd.specdist.multiscale_stft_distance + mel_distance, NumPy float64, one pair at a time in one process
  torch_f32   the reference's arithmetic (torch.stft in float32 with the periodic Hann window, clamp, pow, log10, L1 mean; the mel bank as
              a float32 matmul) on the CPU, one pair at a time
  gpu         specdist.spectral_distances_batch: rows built on the host, copied, scored, read back
  gpu_resident the same native calls on rows already on the device

and for the 4096 scale alone, on resident rows: the fused FFT kernel (a one-scale plan, STFT terms only) against the route the library
had for a spectrum on the GPU before it, fd_metrics_power_spec with a (4096, 1024) plan (the DFT as an exact-float32 GEMM), once per
signal -- which produces the two power spectrograms only, not the distance.  The calibration line (flowdec_amd.boxprobe.calibrate) says
which box it was.

    python scripts/specdist_timing.py [--files 64] [--batch-files 8] [--repeats 5] [--host-repeats 1] [--out profiles/specdist_timing.json]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def torch_f32_distances(x_hat, x, banks):
    st, mel = 0.0, 0.0
    for n_fft, n_mels, has_stft in banks["scales"]:
        win = banks["win"][n_fft]
        A, R = (torch.stft(s, n_fft, hop_length=n_fft // 4, win_length=n_fft, window=win, center=True, pad_mode="reflect", return_complex=True).abs()
                for s in (x_hat, x))
        if has_stft:
            st += float((A.clamp(1e-5).pow(2).log10() - R.clamp(1e-5).pow(2).log10()).abs().mean()) + float((A - R).abs().mean())
        fb = banks["fb"][n_fft]
        Mh, Mx = torch.matmul(A.pow(2).transpose(0, 1), fb), torch.matmul(R.pow(2).transpose(0, 1), fb)
        mel += float((Mh.clamp(1e-5).pow(2).log10() - Mx.clamp(1e-5).pow(2).log10()).abs().mean())
    return st, mel


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=64)
    ap.add_argument("--min-s", type=float, default=1.0)
    ap.add_argument("--max-s", type=float, default=4.0)
    ap.add_argument("--batch-files", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--host-repeats", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "specdist_timing.json"))
    args = ap.parse_args()
    from flowdec_amd import _lib as L, boxprobe, metrics, ops, specdist
    from flowdec_amd.batching import padded_rows

    sr = 48000
    rng = np.random.default_rng(0)
    lens = rng.integers(int(args.min_s * sr), int(args.max_s * sr) + 1, size=args.files)
    hs, xs = [], []
    for n in lens:
        y = (0.1 * rng.standard_normal(int(n))).astype(np.float32)
        x = (y + 0.05 * rng.standard_normal(int(n))).astype(np.float32)
        hs.append(torch.from_numpy((x + 0.02 * rng.standard_normal(int(n))).astype(np.float32)))
        xs.append(torch.from_numpy(x))
    audio = float(lens.sum()) / sr
    lib = L.load()
    plan = specdist.specdist_plan(sr)
    plan4096 = specdist.SpecdistPlan(sr, ((4096, 0, True),))
    gemm_plan = ops.stft_plan(4096, 1024, "cuda")
    banks = dict(scales=specdist.PLAN_SCALES, win={n: torch.hann_window(n, periodic=True) for n, _, _ in specdist.PLAN_SCALES},
                 fb={n: torch.from_numpy(specdist.mel_filterbank(sr, n, m).astype(np.float32)) for n, m, _ in specdist.PLAN_SCALES})

    def clock(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    staged = []
    for idx in metrics.length_sorted_batches([int(n) for n in lens], args.batch_files):
        B, Lmax = len(idx), max(int(lens[i]) for i in idx)
        (h, _), (x, ln) = (padded_rows([l[i] for i in idx], Lmax, "cuda") for l in (hs, xs))
        nws = max(lib.fd_metrics_specdist_workspace_bytes(plan.handle, B, Lmax), lib.fd_metrics_workspace_bytes(B, Lmax, 4096, 1024))
        T, F = 1 + Lmax // 1024, 2049
        staged.append((idx, h, x, ln, torch.empty(nws, dtype=torch.uint8, device="cuda"), torch.empty(B, 2, dtype=torch.float64, device="cuda"),
                       torch.empty(2, B, T, F, dtype=torch.float32, device="cuda")))

    def resident(p):
        def run():
            out = np.zeros((args.files, 2))
            for idx, h, x, ln, ws, val, _ in staged:
                B, Lmax = x.shape
                L.check(lib.fd_metrics_specdist(p.handle, L.ptr(h), L.ptr(x), L.ptr(ln), B, Lmax, L.ptr(val), None, L.ptr(ws), ws.numel(), L.stream()))
                out[idx] = val.cpu().numpy()
            return out
        return run

    def gemm_route():
        for idx, h, x, ln, ws, val, P in staged:
            B, Lmax = x.shape
            for k, sig in enumerate((h, x)):
                L.check(lib.fd_metrics_power_spec(gemm_plan, L.ptr(sig), L.ptr(ln), B, Lmax, L.ptr(P[k]), L.ptr(ws), ws.numel(), L.stream()))
        return None

    def fft_route():            # the kernels alone, as gemm_route: no read-back inside the loop
        for idx, h, x, ln, ws, val, _ in staged:
            B, Lmax = x.shape
            L.check(lib.fd_metrics_specdist(plan4096.handle, L.ptr(h), L.ptr(x), L.ptr(ln), B, Lmax, L.ptr(val), None, L.ptr(ws), ws.numel(), L.stream()))
        return None

    gpu_sides = {
        "gpu": lambda: specdist.spectral_distances_batch(hs, xs, sr, batch=args.batch_files),
        "gpu_resident": resident(plan),
        "fft_4096_resident": fft_route,
        "gemm_4096_resident_two_power_specs": gemm_route,
    }
    host_sides = {
        "host": lambda: np.array([(specdist.multiscale_stft_distance(h, x), specdist.mel_distance(h, x, sr)) for h, x in zip(hs, xs)]),
        "torch_f32": lambda: np.array([torch_f32_distances(h, x, banks) for h, x in zip(hs, xs)]),
    }
    for fn in gpu_sides.values():           # warm-up: plans, allocator, code objects
        fn()
    times, values = {k: [] for k in list(gpu_sides) + list(host_sides)}, {}
    for r in range(args.repeats):
        for name, fn in gpu_sides.items():
            t, values[name] = clock(fn)
            times[name].append(t)
        if r < args.host_repeats:
            for name, fn in host_sides.items():
                t, values[name] = clock(fn)
                times[name].append(t)
    med = {k: statistics.median(v) for k, v in times.items()}
    rel = lambda a, b: float(np.max(np.abs(a - b) / np.abs(b)))
    frames4096 = int(sum(1 + int(n) // 1024 for n in lens))
    out = {
        "what": "msstft + mel of %d pairs at 48 kHz (%.1f s of audio per signal), loading excluded" % (args.files, audio),
        "device": torch.cuda.get_device_name(0), "files": int(args.files), "audio_seconds": audio, "batch_files": args.batch_files, "repeats": args.repeats,
        "host_repeats": args.host_repeats, "seconds": times, "median_s": med, "min_s": {k: min(v) for k, v in times.items()},
        "pairs_per_second": {k: args.files / med[k] for k in ("gpu", "gpu_resident", "host", "torch_f32")},
        "ratio_host_over_gpu": med["host"] / med["gpu"], "ratio_torch_f32_over_gpu": med["torch_f32"] / med["gpu"],
        "ratio_gemm_over_fft_4096": med["gemm_4096_resident_two_power_specs"] / med["fft_4096_resident"], "frames_4096": frames4096,
        "max_rel_gpu_minus_host": [rel(values["gpu"][:, k], values["host"][:, k]) for k in range(2)],
        "max_rel_torch_f32_minus_host": [rel(values["torch_f32"][:, k], values["host"][:, k]) for k in range(2)],
        "gpu_equals_resident_bits": bool(values["gpu"].tobytes() == values["gpu_resident"].tobytes()),
        "box_calibration": boxprobe.calibrate(),
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
