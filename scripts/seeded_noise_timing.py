"""In-call A/B of the seeded noise path against the torch-noise path (MEASUREMENTS.md, "Seeded sampler noise").

    python scripts/seeded_noise_timing.py [--out profiles/seeded_noise_timing.txt]

Three pairs on one MI355X, each pair in one process with its variants interleaved round by round (after a warm-up of every variant),
device-synchronised host clock, shader clock and package power sampled over the whole timed region of the pair:
  * FlowModel.enhance at BASELINE config 2's shape (FlowDec-75m, 8 x 2 s, Euler-6, bf16): seed= against generator=;
  * sharded_enhance at the same shape (what bench.py times): rng="native" against rng="torch";
  * ScoreModel.enhance (N = 30, one corrector step, 8 x 2 s): seed= against the default, with torch.cuda.max_memory_allocated.
Weights are seeded random numbers (speed does not depend on them)."""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import flowdec_amd  # noqa: E402
from flowdec_amd import boxprobe  # noqa: E402
from flowdec_amd.dist import sharded_enhance  # noqa: E402


def random_weights(m, seed=1234):
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for k, v in m.state_dict().items():
        if not k.startswith("backbone."):
            continue
        if k.endswith(".W"):
            sd[k] = torch.randn(v.shape, generator=g) * 16.0
        elif v.ndim == 1 and k.endswith("weight"):
            sd[k] = 1.0 + 0.1 * torch.randn(v.shape, generator=g)
        elif k.endswith("bias"):
            sd[k] = 0.05 * torch.randn(v.shape, generator=g)
        else:
            sd[k] = torch.randn(v.shape, generator=g) / v[0].numel() ** 0.5
    m.load_state_dict(sd, strict=False)
    return m.cuda()


def ab(name, variants, rounds, warmup, lines):
    """variants: {label: fn(k)}; every round runs each variant once, in order; -> per-variant mean / min ms."""
    for k in range(warmup):
        for fn in variants.values():
            fn(k)
    torch.cuda.synchronize()
    times = {label: [] for label in variants}
    with boxprobe.PowerSampler(0, period_s=0.1) as ps:
        for k in range(rounds):
            for label, fn in variants.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn(warmup + k)
                torch.cuda.synchronize()
                times[label].append(1e3 * (time.perf_counter() - t0))
    power = ps.summary()
    for label, t in times.items():
        lines.append(f"{name:34s} {label:22s} mean {np.mean(t):9.3f} ms  min {np.min(t):9.3f} ms  median {np.median(t):9.3f} ms  ({len(t)} rounds)")
    lines.append(f"{name:34s} clock / power over the pair: {power}")
    print("\n".join(lines[-len(times) - 1:]), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "seeded_noise_timing.txt"))
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--score-rounds", type=int, default=4)
    args = ap.parse_args()
    lines = [f"seeded noise timing: {torch.cuda.get_device_name(0)}, torch {torch.__version__}"]
    y = 0.1 * torch.randn(8, 1, 96000, device="cuda", generator=torch.Generator(device="cuda").manual_seed(0))

    flow = random_weights(flowdec_amd.from_preset("flowdec_75m", precision="bf16"))
    ab("enhance 8x2s euler-6 bf16", {
        "generator=": lambda k: flow.enhance(y, N=6, solver="euler", generator=torch.Generator(device="cuda").manual_seed(1000 + k)),
        "seed=": lambda k: flow.enhance(y, N=6, solver="euler", seed=1000 + k),
    }, args.rounds, 3, lines)
    ab("sharded_enhance 8x2s euler-6 bf16", {
        "rng=torch": lambda k: sharded_enhance(flow, y, N=6, solver="euler", seed=1000 + k),
        "rng=native": lambda k: sharded_enhance(flow, y, N=6, solver="euler", seed=1000 + k, rng="native"),
    }, args.rounds, 3, lines)
    del flow
    torch.cuda.empty_cache()

    score = random_weights(flowdec_amd.from_preset("baseline_scoredec_75s", precision="bf16"))
    kw = dict(N=30, predictor="reverse_diffusion", corrector="ald", corrector_steps=1)
    peak = {}
    for label, call in (("seed=", lambda k: score.enhance(y, seed=k, **kw)), ("default (torch.randn)", lambda k: score.enhance(y, **kw))):
        score._io = {}
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        call(0)
        torch.cuda.synchronize()
        peak[label] = torch.cuda.max_memory_allocated()
    lines.append("ScoreModel.enhance N=30 8x2s: torch.cuda.max_memory_allocated " + ", ".join(f"{k}: {v / 2 ** 20:.1f} MiB" for k, v in peak.items()))
    print(lines[-1], flush=True)
    # (each variant keeps its own io buffers: _wave_call holds one shape, so the interleaved pair re-allocates -- time them in blocks)
    for label, call in (("default (torch.randn)", lambda k: score.enhance(y, **kw)), ("seed=", lambda k: score.enhance(y, seed=k, **kw)),
                        ("default (torch.randn) again", lambda k: score.enhance(y, **kw)), ("seed= again", lambda k: score.enhance(y, seed=k, **kw))):
        ab("ScoreModel.enhance N=30 8x2s bf16", {label: call}, args.score_rounds, 2, lines)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
