"""Streaming enhance: pooled throughput against `enhance_long`, and the host cost of a step (MEASUREMENTS.md, "Streaming enhance").

    python scripts/stream_timing.py [--out profiles/stream_timing.txt] [--rows 20] [--rounds 3]

One MI355X, one process, FlowDec-75m with seeded random weights, bf16, Euler-6, rows of 256 frames with halos of 64 (W = 98 303 samples =
2.05 s, stride 1.016 s), a fixed normalisation factor on both sides.  For 1 and for 8 sessions, interleaved in one process (stream,
long, stream, long, ...; device-synchronised host clock; both warmed up twice, the second pass captures the graphs):
  * stream: a `StreamPool` of that many sessions fed in lockstep, 4800 samples (0.1 s) per push from device memory, one `step()` per round
    of pushes, `flush_many` at the end;
  * long: `enhance_long` on the same audio ([sessions, 1, n]) with the same geometry and `rows_per_call` = sessions: the same number of
    native calls of the same batch size.
Then, in a pass of its own, the host time of one `step()` with the device idle before it (table build, the one upload, the three
enqueues), and the delay formula beside the measured time of a row.  The outputs are compared bit for bit before anything is timed."""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import flowdec_amd  # noqa: E402
from flowdec_amd.stream import StreamPool  # noqa: E402
from seeded_noise_timing import random_weights  # noqa: E402

SR, HOP, RF, HALO, BLOCK = 48000, 384, 256, 64, 4800
KW = dict(N=6, solver="euler", row_frames=RF, halo_frames=HALO)
NORMFAC = 0.5


def run_stream(pool, ys, seeds, host_times=None):
    """Every channel of ys [S, n] as one session of `pool`, in lockstep -> ([S, n] output, native calls)."""
    S, n = ys.shape
    sids = [pool.open([s]) for s in seeds]
    outs = {sid: [] for sid in sids}
    calls0 = pool.native_calls
    for pos in range(0, n, BLOCK):
        for c, sid in enumerate(sids):
            pool.push(sid, ys[c, pos:pos + BLOCK])
        if host_times is not None:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
        got = pool.step()
        if host_times is not None and got:
            host_times.append(time.perf_counter() - t0)
        for sid, o in got.items():
            outs[sid].append(o)
    for sid, o in pool.flush_many(sids).items():
        outs[sid].append(o)
    return torch.stack([torch.cat(outs[sid]) for sid in sids]), pool.native_calls - calls0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stream_timing.txt"))
    ap.add_argument("--rows", type=int, default=20, help="rows per session")
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    lines = [f"stream timing: {torch.cuda.get_device_name(0)}, torch {torch.__version__}"]

    def say(s):
        lines.append(s)
        print(s, flush=True)

    W, stride, half = RF * HOP - 1, (RF - 2 * HALO - 1) * HOP, HOP
    n = (args.rows - 1) * stride + W - 1000
    delay = (RF - HALO) * HOP + half
    model = random_weights(flowdec_amd.from_preset("flowdec_75m", precision="bf16"))
    g = torch.Generator(device="cuda").manual_seed(0)
    say(f"bf16, Euler-6, rows of {RF} frames (W = {W} samples = {W / SR:.3f} s), halo {HALO}, stride {stride} samples = {stride / SR:.3f} s; "
        f"{n} samples = {n / SR:.1f} s = {args.rows} rows per session; pushes of {BLOCK} samples; normfac {NORMFAC}")
    for S in (1, 8):
        ys = 0.1 * torch.randn(S, n, device="cuda", generator=g)
        seeds = [1000 + c for c in range(S)]
        pool = StreamPool(model, capacity=S, normfac=NORMFAC, **KW)          # ONE pool for every pass: its buffers key the graphs
        stream = lambda: run_stream(pool, ys, seeds)
        long = lambda: model.enhance_long(ys[:, None], seed=seeds, normfac=NORMFAC, rows_per_call=S, **KW)
        a, calls = stream()
        b = long()[:, 0]
        say(f"{S} session(s): stream == enhance_long bit for bit: {torch.equal(a, b)}; native calls per pass: {calls}")
        stream(), long()
        ts, tl = [], []
        for _ in range(args.rounds):
            for fn, t in ((stream, ts), (long, tl)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                t.append(time.perf_counter() - t0)
        ms, ml = float(np.mean(ts)), float(np.mean(tl))
        audio = S * n / SR
        say(f"  stream       : mean {ms * 1e3:9.1f} ms  min {min(ts) * 1e3:9.1f} ms  -> {audio / ms:7.1f} x real time  ({ms / calls * 1e3:7.2f} ms per native call)")
        say(f"  enhance_long : mean {ml * 1e3:9.1f} ms  min {min(tl) * 1e3:9.1f} ms  -> {audio / ml:7.1f} x real time  ({ml / calls * 1e3:7.2f} ms per native call)")
        say(f"  throughput ratio stream / enhance_long: {ml / ms:.4f} (means), {min(tl) / min(ts):.4f} (minima); difference per native call "
            f"{(ms - ml) / calls * 1e3:+.3f} ms")
        host = []
        run_stream(pool, ys, seeds, host)
        say(f"  host time of one step() with the device idle before it (table, upload, three enqueues): median {np.median(host) * 1e3:.3f} ms, "
            f"max {max(host) * 1e3:.3f} ms over {len(host)} steps")
        row = ml / calls
        say(f"  delay: a sample leaves once (row_frames - halo_frames) * hop + xfade / 2 = {delay} further samples ({delay / SR:.3f} s) have "
            f"arrived, plus the compute time of a call of {S} row(s): {row * 1e3:.1f} ms -> {delay / SR + row:.3f} s worst case")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
