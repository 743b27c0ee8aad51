"""Long-form and streaming for the ScoreDec and regression baselines: what they cost (MEASUREMENTS.md, "Baselines: long-form and streaming").

    python scripts/baselines_longform_timing.py [--out profiles/baselines_longform_timing.txt] [--parent-tree DIR] [--parts 1,2,3]

One MI355X, bf16, the flowdec_75m-width backbone with seeded random weights (speed does not depend on them), device-synchronised host clock.
  1. The existing path: `ScoreModel.enhance_batch(seeds=)` on 8 x 2 s, N = 30, one ald step -- its prior and its 60 fused updates run the two
     kernels that gained the frame0 argument.  A library cannot be swapped inside a process, so the interleaving is one of processes: parent,
     this, parent, this, ... (`--parent-tree`: a built checkout of the parent commit; without it the part is skipped).  The margin is the
     spread between the parent's own runs.
  2. Long-form against one clip: the class's long form (`_WaveModel._enhance_long`, default rows of 3712 frames, halos of 256) on a 5-minute
     recording against `enhance` of one 30 s clip, per second of audio.  Predicted: the halo share, 3712 / (3712 - 513) = 1.16.
  3. Streaming: 1 and 8 sessions of a `StreamPool` against the long form on the same audio at rows of 256 frames / halos of 64 (the layout of
     scripts/stream_timing.py), and from the regression model's one-row call its end-to-end delay."""
import argparse
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--parent-tree", default=None, help="a built checkout of the parent commit (part 1)")
ap.add_argument("--parts", default="1,2,3")
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--pairs", type=int, default=3, help="part 1: processes per library")
ap.add_argument("--N", type=int, default=30, help="reverse steps of the score sampler in parts 2 and 3")
ap.add_argument("--rows", type=int, default=6, help="part 3: rows per session")
ap.add_argument("--worker", default=None, help="internal: run part 1's timing in this process against the tree --tree")
ap.add_argument("--tree", default=os.path.dirname(HERE))
args = ap.parse_args()
ROOT = os.path.abspath(args.tree)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402

SR, HOP = 48000, 384
torch = flowdec_amd = random_weights = None


def heavy_imports():
    """torch and the package, from --tree.  Part 1's driver runs before them: it only starts fresh child processes, and must not hold the GPU."""
    global torch, flowdec_amd, random_weights
    import torch
    import flowdec_amd
    from seeded_noise_timing import random_weights


OUT = args.out or os.path.join(os.path.dirname(HERE), "profiles", "baselines_longform_timing.txt")


def say(s):
    print(s, flush=True)
    if not args.worker:
        with open(OUT, "a") as f:
            f.write(s + "\n")


def timed(fn, rounds, warmup=1):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return ts


def build(kind):
    return random_weights(flowdec_amd.from_preset({"score": "baseline_scoredec_75s", "regression": "baseline_regression_75s"}[kind], precision="bf16"))


def sampler_of(kind):
    return dict(N=args.N, predictor="reverse_diffusion", corrector="ald", corrector_steps=1) if kind == "score" else {}


def worker_existing():
    """Part 1 in one process, against the tree this process imported: prints `mean min` in ms."""
    heavy_imports()
    m = build("score")
    g = torch.Generator(device="cuda").manual_seed(0)
    clips = [0.1 * torch.randn(96000, device="cuda", generator=g) for _ in range(8)]
    kw = dict(N=30, predictor="reverse_diffusion", corrector="ald", corrector_steps=1)
    ts = timed(lambda: m.enhance_batch(clips, seeds=list(range(100, 108)), **kw), args.rounds, warmup=2)
    print(f"RESULT {1e3 * np.mean(ts):.3f} {1e3 * np.min(ts):.3f}", flush=True)


def part1():
    if not args.parent_tree:
        say("1. existing path: skipped (no --parent-tree)")
        return
    res = {"parent": [], "this": []}
    for k in range(args.pairs):
        for label, tree in (("parent", args.parent_tree), ("this", ROOT)):
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", "existing", "--tree", tree, "--rounds", str(args.rounds)],
                                 capture_output=True, text=True, timeout=240, check=True).stdout
            mean, mn = [float(v) for v in [l for l in out.splitlines() if l.startswith("RESULT")][0].split()[1:]]
            res[label].append((mean, mn))
            say(f"1. ScoreModel.enhance_batch(seeds=) 8 x 2 s, N = 30, ald: {label:6s} process {k}: mean {mean:9.3f} ms  min {mn:9.3f} ms ({args.rounds} rounds)")
    pm, tm = [r[1] for r in res["parent"]], [r[1] for r in res["this"]]
    say(f"1. minima: parent {min(pm):.3f} .. {max(pm):.3f} ms (spread between the parent's own processes {max(pm) - min(pm):.3f} ms = "
        f"{100 * (max(pm) - min(pm)) / min(pm):.2f} %), this {min(tm):.3f} .. {max(tm):.3f} ms; this / parent (medians of the minima) = "
        f"{np.median(tm) / np.median(pm):.4f}")


def part2():
    g = torch.Generator(device="cuda").manual_seed(1)
    clip = 0.1 * torch.randn(30 * SR - 1000, device="cuda", generator=g)
    rec = 0.1 * torch.randn(300 * SR, device="cuda", generator=g)
    for kind in ("regression", "score"):
        m, kw = build(kind), sampler_of(kind)
        call = m._chunks_call(**kw)
        seed = dict(seed=5) if kind == "score" else {}
        tc = timed(lambda: m.enhance(clip, **seed, **kw), args.rounds)
        tl = timed(lambda: m._enhance_long(rec, call, seed=5), max(1, args.rounds - 1))
        rows = m._enhance_long_jobs(rec)
        per_s_clip, per_s_long = min(tc) / (clip.numel() / SR), min(tl) / 300.0
        say(f"2. {kind:10s} {kw or ''}: enhance of {clip.numel() / SR:.2f} s: min {1e3 * min(tc):9.1f} ms; long form of 300 s ({rows} rows, 8 per call): "
            f"min {1e3 * min(tl):9.1f} ms; cost per second of audio long / clip = {per_s_long / per_s_clip:.3f} (predicted 1.16; flow model: measured 1.11)")
        del m
        torch.cuda.empty_cache()


def part3():
    from flowdec_amd.stream import StreamPool
    from stream_timing import BLOCK, HALO, NORMFAC, RF, run_stream
    geo = dict(row_frames=RF, halo_frames=HALO)
    W, stride = RF * HOP - 1, (RF - 2 * HALO - 1) * HOP
    n = (args.rows - 1) * stride + W - 1000
    delay = (RF - HALO) * HOP + HOP
    g = torch.Generator(device="cuda").manual_seed(2)
    say(f"3. rows of {RF} frames (W = {W} samples), halo {HALO}; {n} samples = {n / SR:.1f} s = {args.rows} rows per session; pushes of {BLOCK}; normfac {NORMFAC}")
    for kind in ("regression", "score"):
        m, kw = build(kind), sampler_of(kind)
        call = m._chunks_call(**kw)
        for S in (1, 8):
            ys = 0.1 * torch.randn(S, n, device="cuda", generator=g)
            seeds = [1000 + c for c in range(S)]
            pool = StreamPool(m, capacity=S, normfac=NORMFAC, **geo, **kw)
            stream = lambda: run_stream(pool, ys, seeds)
            long = lambda: m._enhance_long(ys[:, None], call, seed=seeds, normfac=NORMFAC, rows_per_call=S, **geo)
            (a, calls), b = stream(), long()[:, 0]
            ts, tl = timed(stream, args.rounds), timed(long, args.rounds)
            audio = S * n / SR
            say(f"3. {kind:10s} {S} session(s): stream == long form bit for bit: {torch.equal(a, b)}; {calls} native calls; stream min {1e3 * min(ts):9.1f} ms "
                f"({audio / min(ts):7.1f} x real time), long form min {1e3 * min(tl):9.1f} ms ({audio / min(tl):7.1f} x); stream / long = {min(ts) / min(tl):.4f}; "
                f"one call of {S} row(s): {1e3 * min(tl) / calls:.2f} ms")
            if S == 1:
                row = min(tl) / calls
                say(f"3. {kind:10s} end-to-end delay of one stream: (rf - halo) * hop + xfade / 2 = {delay} samples = {1e3 * delay / SR:.1f} ms, plus one row's "
                    f"call {1e3 * row:.2f} ms -> {1e3 * (delay / SR + row):.1f} ms")
        del m
        torch.cuda.empty_cache()


if __name__ == "__main__":
    if args.worker == "existing":
        worker_existing()
        sys.exit(0)
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    open(OUT, "w").close()
    parts = args.parts.split(",")
    if "1" in parts:
        part1()
    heavy_imports()
    say(f"baselines long-form timing: {torch.cuda.get_device_name(0)}, torch {torch.__version__}, bf16, flowdec_75m-width backbone, random weights")
    for p, fn in (("2", part2), ("3", part3)):
        if p in parts:
            fn()
