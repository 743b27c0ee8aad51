"""Long-form enhance: rate and seam report (MEASUREMENTS.md, "Long-form enhance").

    python scripts/long_form_timing.py [--out profiles/long_form_timing.txt] [--minutes 10]

One MI355X, one process, FlowDec-75m with seeded random weights:
  * rate: `enhance_long` on one 10-minute clip (bf16, Euler-6, the default rows of 3712 frames with halos of 256, 8 rows per call)
    against `enhance` on a 30 s clip; device-synchronised host clock, every variant warmed up twice (the second call captures the graph).
    Expected: the 30 s one-shot rate divided by the halo share row_frames / (row_frames - 2 halo_frames - 1) = 1.16.
  * seam report: on a 60 s clip, which fits both ways, in fp32: the relative L2 difference between `enhance_long` (three rows) and
    `enhance(seed=)` (one image) with the same seed, split into the samples within one halo of a row boundary and the samples elsewhere.
    The two share the noise and the normalisation factor; they differ through the GroupNorm statistics (per row against per file) and
    through edge effects at the rows' ends.  A profile in 2-second bins follows.  Random weights are chaotic: the figure says little about
    trained ones.
Nothing is asserted."""
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
from flowdec_amd import _lib as L  # noqa: E402
from flowdec_amd import longform  # noqa: E402
from seeded_noise_timing import random_weights  # noqa: E402

SR, HOP = 48000, 384


def timed(fn, warmup, rounds):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t = []
    for _ in range(rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        t.append(time.perf_counter() - t0)
    return float(np.mean(t)), float(np.min(t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "long_form_timing.txt"))
    ap.add_argument("--minutes", type=float, default=10.0)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--seam-seconds", type=float, default=60.0)
    args = ap.parse_args()
    lines = [f"long-form timing: {torch.cuda.get_device_name(0)}, torch {torch.__version__}"]

    def say(s):
        lines.append(s)
        print(s, flush=True)

    g = torch.Generator(device="cuda").manual_seed(0)
    rf, halo = 3712, 256
    share = rf / (rf - 2 * halo - 1)

    # ---- rate -------------------------------------------------------------------------------------------------------------------------
    flow = random_weights(flowdec_amd.from_preset("flowdec_75m", precision="bf16"))
    y30 = 0.1 * torch.randn(30 * SR, device="cuda", generator=g)
    ylong = 0.1 * torch.randn(int(args.minutes * 60 * SR), device="cuda", generator=g)
    rows = longform.plan_rows(ylong.numel(), HOP, rf, halo)
    lib, h = L.load(), flow._sync_native()
    ws_rows = lib.fd_enhance_workspace_bytes(h, 8, longform.row_samples(rf, HOP))
    ws_one = lib.fd_enhance_workspace_bytes(h, 1, ylong.numel())
    say(f"{args.minutes:g} min = {ylong.numel()} samples = {len(rows)} rows of {rf} frames (halo {halo}); workspace (computed): 8 rows "
        f"{ws_rows / 1e9:.2f} GB, the same clip in one call {ws_one / 1e9:.2f} GB")
    mean30, min30 = timed(lambda: flow.enhance(y30, N=6, solver="euler", seed=1), 2, args.rounds)
    say(f"enhance       30 s, bf16, Euler-6:  mean {mean30 * 1e3:9.1f} ms  min {min30 * 1e3:9.1f} ms  -> {30 / mean30:7.1f} x real time")
    flow._io = {}
    torch.cuda.empty_cache()
    secs = ylong.numel() / SR
    meanL, minL = timed(lambda: flow.enhance_long(ylong, N=6, solver="euler", seed=1), 2, args.rounds)
    say(f"enhance_long {secs:5.0f} s, bf16, Euler-6:  mean {meanL * 1e3:9.1f} ms  min {minL * 1e3:9.1f} ms  -> {secs / meanL:7.1f} x real time")
    say(f"cost over the 30 s one-shot rate: {(meanL / secs) / (mean30 / 30):.3f} (expected: the halo share {share:.3f}; rows actually run per "
        f"row's worth of kept audio: {len(rows) * longform.row_samples(rf, HOP) / ylong.numel():.3f})")
    say(f"torch.cuda.max_memory_allocated: {torch.cuda.max_memory_allocated() / 1e9:.2f} GB")
    del flow, ylong, y30
    torch.cuda.empty_cache()

    # ---- seam report ---------------------------------------------------------------------------------------------------------------------
    f32 = random_weights(flowdec_amd.from_preset("flowdec_75m", precision="fp32"))
    y = 0.1 * torch.randn(int(args.seam_seconds * SR), device="cuda", generator=g)
    rows = longform.plan_rows(y.numel(), HOP, rf, halo)
    one = f32.enhance(y, N=6, solver="euler", seed=7).double()
    lng = f32.enhance_long(y, N=6, solver="euler", seed=7).double()
    near = torch.zeros(y.numel(), dtype=torch.bool, device="cuda")
    for r in rows[1:]:
        near[max(r.xfade_lo - halo * HOP, 0):r.xfade_lo + halo * HOP] = True

    def rel(mask):
        return float(((lng - one)[mask].norm() / one[mask].norm()).item())

    say(f"seam report, fp32, Euler-6, {args.seam_seconds:g} s = {len(rows)} rows, boundaries at samples {[r.xfade_lo for r in rows[1:]]}:")
    say(f"  relative L2 of enhance_long against enhance(seed=): within one halo ({halo} frames) of a boundary {rel(near):.3e} "
        f"({int(near.sum())} samples), elsewhere {rel(~near):.3e} ({int((~near).sum())} samples), whole clip {rel(torch.ones_like(near)):.3e}")
    x = 2 * HOP
    for r in rows[1:]:
        c = r.xfade_lo
        say(f"  boundary {c}: relative L2 inside the cross-fade ({x} samples) {float(((lng - one)[c - x // 2:c + x // 2].norm() / one[c - x // 2:c + x // 2].norm()).item()):.3e}")
    # where along the clip the two differ: 2-second bins (rms of each output and the relative L2 of the difference)
    say("  per 2 s of the clip: start [s], rms enhance, rms enhance_long, relative L2")
    for lo in range(0, y.numel(), 2 * SR):
        a, b = one[lo:lo + 2 * SR], lng[lo:lo + 2 * SR]
        say(f"    {lo / SR:5.1f}  {float(a.square().mean().sqrt()):.3e}  {float(b.square().mean().sqrt()):.3e}  {float((b - a).norm() / a.norm()):.3e}")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
