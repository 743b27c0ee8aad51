"""Device resampler timing (MEASUREMENTS.md, "Device resampler"): host `audio.resample` against `resample_device`, what the float64
contract costs, and the two places the resampler is wired in.

    python scripts/resample_timing.py [--seconds 30] [--repeats 20] [--f32-lib PATH] [--skip-eval] [--skip-stream] [--out profiles/resample_timing.json]

One MI355X, one process; A and B of every comparison alternate inside one loop after a warm-up; host clock around work that ends in a
device synchronise, device events for the kernel alone; medians.

1. `--seconds` of mono noise, 44.1 -> 48 kHz, lowpass_filter_width 64 and 256: the host resampler (torch conv1d on the CPU, torch's
   thread count as found) against `resample_device` with and without the host-to-device copy (pageable memory, as the command lines
   hold it), and fd_resample alone against a float32-ACCUMULATING build of the same kernel (-DFD_RESAMPLE_ACC=float: a timing build,
   not shipped; `build_f32_variant` compiles it when --f32-lib does not exist).
2. `eval_cli` on the 64-file corpus of scripts/eval_timing.py written at 44.1 kHz: --resample host against device, wall time of the run.
3. `EnhanceStream` (FlowDec-75m, random weights, bf16, Euler-6, rows of 256 frames) fed 0.1 s blocks at 44.1 kHz with in_rate=44100
   against the model-rate stream of scripts/stream_timing.py: host time of a push that runs a row, of a push that does not, and the
   delay the resampler adds."""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

F32_LIB = os.path.join(ROOT, "flowdec_amd", "variants", "libflowdec_resample_f32.so")


def build_f32_variant(path):
    """resample.hip with a float32 accumulator + api.hip (the error plumbing) -> a library of its own."""
    from flowdec_amd import build as B
    os.makedirs(os.path.dirname(path), exist_ok=True)
    cmd = [B._hipcc(), *B.FLAGS, "-DFD_RESAMPLE_ACC=float", "-shared", os.path.join(B.CSRC, "resample.hip"), os.path.join(B.CSRC, "api.hip"), "-o", path]
    subprocess.run(cmd, check=True)
    return path


def bind(path):
    from flowdec_amd import _lib as L
    lib = C.CDLL(path)
    for name in ("fd_resample_plan_create", "fd_resample_plan_destroy", "fd_resample", "fd_last_error"):
        res, args = L.SIGNATURES[name]
        getattr(lib, name).restype, getattr(lib, name).argtypes = res, args
    return lib


def median_ms(ts):
    return 1e3 * statistics.median(ts)


def host_clock(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def one_shot(args, say):
    from flowdec_amd import _lib as L
    from flowdec_amd.audio import resample, sinc_resample_kernel
    from flowdec_amd.resample import get_resampler, resample_device
    lib64, lib32 = L.load(), bind(args.f32_lib if os.path.exists(args.f32_lib) else build_f32_variant(args.f32_lib))
    n_in = int(args.seconds * 44100)
    x = torch.from_numpy((0.1 * np.random.default_rng(0).standard_normal((1, n_in))).astype(np.float32))
    xd = x.cuda()
    out = []
    for lpw in (64, 256):
        r = get_resampler(44100, 48000, lpw, device="cuda:0")
        M = r.out_length(n_in)
        bank, width, o, n = sinc_resample_kernel(44100, 48000, lpw)
        plan32 = C.c_void_p()
        assert lib32.fd_resample_plan_create(np.ascontiguousarray(bank).ctypes.data_as(C.c_void_p), o, n, width, C.byref(plan32)) == 0, lib32.fd_last_error()
        y64, y32 = torch.empty(1, M, device="cuda"), torch.empty(1, M, device="cuda")
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

        def kernel(lib, plan, y):
            ev[0].record()
            rc = lib.fd_resample(plan, L.ptr(xd), None, 1, n_in, L.ptr(y), M, L.stream())
            ev[1].record()
            ev[1].synchronize()
            assert rc == 0
            return ev[0].elapsed_time(ev[1])

        host_y = resample(x, 44100, 48000, lowpass_filter_width=lpw)
        dev_y = resample_device(xd, 44100, 48000, lowpass_filter_width=lpw)
        kernel(lib64, r._plan, y64), kernel(lib32, plan32, y32)
        assert torch.equal(dev_y, y64)
        t = dict(host=[], dev_h2d=[], dev=[], k64=[], k32=[])
        for _ in range(args.repeats):
            t["host"].append(host_clock(lambda: resample(x, 44100, 48000, lowpass_filter_width=lpw))[0])
            t["dev_h2d"].append(host_clock(lambda: resample_device(x.cuda(), 44100, 48000, lowpass_filter_width=lpw))[0])
            t["dev"].append(host_clock(lambda: resample_device(xd, 44100, 48000, lowpass_filter_width=lpw))[0])
            t["k64"].append(1e-3 * kernel(lib64, r._plan, y64))
            t["k32"].append(1e-3 * kernel(lib32, plan32, y32))
        lib32.fd_resample_plan_destroy(plan32)
        macs = M * (2 * width + o)
        row = dict(lowpass_filter_width=lpw, K=2 * width + o, input_samples=n_in, output_samples=M, multiply_adds=macs,
                   host_ms=median_ms(t["host"]), device_with_h2d_ms=median_ms(t["dev_h2d"]), device_ms=median_ms(t["dev"]),
                   kernel_f64_ms=median_ms(t["k64"]), kernel_f32_timing_build_ms=median_ms(t["k32"]),
                   kernel_f64_min_ms=1e3 * min(t["k64"]), kernel_f32_min_ms=1e3 * min(t["k32"]),
                   kernel_f64_gmacs_per_s=macs / statistics.median(t["k64"]) / 1e9,
                   max_abs_device_minus_host=float((dev_y.cpu() - host_y).abs().max()), max_abs_f32_build_minus_f64=float((y32 - y64).abs().max()))
        out.append(row)
        say(f"{args.seconds:g} s mono 44.1 -> 48 kHz, lowpass_filter_width {lpw} (K = {row['K']}, {macs / 1e6:.0f} M multiply-adds), medians of {args.repeats}: "
            f"host {row['host_ms']:.2f} ms ({torch.get_num_threads()} threads) | device with H2D {row['device_with_h2d_ms']:.2f} ms, without "
            f"{row['device_ms']:.2f} ms | kernel alone: float64 {row['kernel_f64_ms']:.3f} ms, float32 timing build {row['kernel_f32_timing_build_ms']:.3f} ms "
            f"(x{row['kernel_f64_ms'] / row['kernel_f32_timing_build_ms']:.2f})")
    return out


def eval_corpus(args, say):
    from flowdec_amd import eval_cli
    from flowdec_amd.audio import save_wav
    rng = np.random.default_rng(0)
    lens = rng.integers(44100, 4 * 44100 + 1, size=args.files)
    with tempfile.TemporaryDirectory() as d:
        lines = []
        for i, n in enumerate(lens):
            y = (0.1 * rng.standard_normal(int(n))).astype(np.float32)
            x = (y + 0.05 * rng.standard_normal(int(n))).astype(np.float32)
            h = (x + 0.02 * rng.standard_normal(int(n))).astype(np.float32)
            paths = [os.path.join(d, f"{k}_{i:03d}.wav") for k in ("clean", "noisy", "enh")]
            for p, s in zip(paths, (x, y, h)):
                save_wav(p, torch.from_numpy(s), 44100)
            lines.append(" ---> ".join(paths))
        lst = os.path.join(d, "triples_list.txt")
        with open(lst, "w") as f:
            f.write("\n".join(lines) + "\n")

        def run(mode):
            return host_clock(lambda: eval_cli.run(["--triples", lst, "--out", os.path.join(d, f"{mode}.csv"), "--resample", mode]))

        stdout, sys.stdout = sys.stdout, open(os.devnull, "w")
        try:
            run("device"), run("host")
            th, td = [], []
            for _ in range(3):
                t, res_h = run("host")
                th.append(t)
                t, res_d = run("device")
                td.append(t)
        finally:
            sys.stdout.close()
            sys.stdout = stdout
    row = dict(files=int(args.files), audio_seconds_per_signal=float(lens.sum()) / 44100, host_s=th, device_s=td, host_median_s=statistics.median(th),
               device_median_s=statistics.median(td), means_host=[m[1] for m in res_h.means], means_device=[m[1] for m in res_d.means])
    say(f"eval_cli, {args.files} triples at 44.1 kHz ({row['audio_seconds_per_signal']:.0f} s per signal, 3 signals each resampled at width 256), wall time of "
        f"the whole run, medians of 3: --resample host {row['host_median_s']:.3f} s | --resample device {row['device_median_s']:.3f} s "
        f"(x{row['host_median_s'] / row['device_median_s']:.2f})")
    return row


def stream(args, say):
    import flowdec_amd
    from flowdec_amd.stream import EnhanceStream
    from seeded_noise_timing import random_weights
    RF, HALO, HOP = 256, 64, 384
    kw = dict(N=6, solver="euler", row_frames=RF, halo_frames=HALO, normfac=0.5)
    model = random_weights(flowdec_amd.from_preset("flowdec_75m", precision="bf16"))
    W, stride = RF * HOP - 1, (RF - 2 * HALO - 1) * HOP
    n48 = (args.rows - 1) * stride + W - 1000
    g = torch.Generator(device="cuda").manual_seed(0)
    y48 = 0.1 * torch.randn(n48, device="cuda", generator=g)
    y44 = 0.1 * torch.randn(-(-n48 * 147 // 160), device="cuda", generator=g)

    def run(y, block, in_rate, host=None):
        st = EnhanceStream(model, seed=[1000], in_rate=in_rate, **kw)
        rows0 = st.pool.rows_run
        for pos in range(0, y.numel(), block):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            st.push(y[pos:pos + block])
            dt = time.perf_counter() - t0
            if host is not None:
                host[st.pool.rows_run > rows0].append(dt)
            rows0 = st.pool.rows_run
        st.flush()
        return st

    out = {}
    for name, y, block, rate in (("model rate", y48, 4800, None), ("in_rate 44100", y44, 4410, 44100)):
        run(y, block, rate), run(y, block, rate)                      # warm-up: the second pass replays the graphs
    for name, y, block, rate in (("model rate", y48, 4800, None), ("in_rate 44100", y44, 4410, 44100)) * 2:
        host = {True: [], False: []}
        wall, st = host_clock(lambda: run(y, block, rate, host))
        o = out.setdefault(name, dict(wall_s=[], push_with_row_ms=[], push_without_row_ms=[]))
        o["wall_s"].append(wall)
        o["push_with_row_ms"] += [1e3 * t for t in host[True]]
        o["push_without_row_ms"] += [1e3 * t for t in host[False]]
        o["delays"] = list(st.delays)
    for name, o in out.items():
        o["push_with_row_median_ms"], o["push_without_row_median_ms"] = statistics.median(o["push_with_row_ms"]), statistics.median(o["push_without_row_ms"])
        say(f"EnhanceStream, {name}: host time of a push (device idle before it) that runs a row: median {o['push_with_row_median_ms']:.3f} ms "
            f"over {len(o['push_with_row_ms'])}; that runs none: median {o['push_without_row_median_ms']:.3f} ms over {len(o['push_without_row_ms'])}; "
            f"whole stream {statistics.median(o['wall_s']):.3f} s; delays (in, pool, out) = {o['delays']} samples")
        del o["push_with_row_ms"], o["push_without_row_ms"]
    d = out["in_rate 44100"]["delays"][0]
    say(f"added delay of the input resampler: {d} samples at 44.1 kHz = {1e3 * d / 44100:.2f} ms, beside the pool's "
        f"{out['in_rate 44100']['delays'][1]} samples = {1e3 * out['in_rate 44100']['delays'][1] / 48000:.1f} ms")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=30.0)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--files", type=int, default=64)
    ap.add_argument("--rows", type=int, default=8, help="rows of the stream comparison")
    ap.add_argument("--f32-lib", default=F32_LIB)
    ap.add_argument("--skip-eval", action="store_true")
    ap.add_argument("--skip-stream", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resample_timing.json"))
    args = ap.parse_args()
    lines = []

    def say(s):
        lines.append(s)
        print(s, flush=True)

    out = dict(device=torch.cuda.get_device_name(0), torch=torch.__version__, host_threads=torch.get_num_threads())
    out["one_shot"] = one_shot(args, say)
    if not args.skip_eval:
        out["eval_cli"] = eval_corpus(args, say)
    if not args.skip_stream:
        out["stream"] = stream(args, say)
    out["lines"] = lines
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
