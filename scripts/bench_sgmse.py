#!/usr/bin/env python
"""Throughput of the SGMSE-style backbone (from_preset("flow_model_sgmse"): nf 128, seven levels, bottleneck attention, 3x3 output
layer) with the timed-region rules of bench.py: seeded random-init weights, the batch resident in HBM before the timed region, the
initial noise drawn inside every call (sharded_enhance(seed=1000 + step)), hipGraph replay, warm-up steps outside the region, one
device synchronisation at each end.  Prints one JSON line.

    python scripts/bench_sgmse.py [--batch 8] [--seconds 2] [--N 3] [--solver midpoint] [--steps 5] [--warmup 2] [--precision bf16]
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--seconds", type=float, default=2.0)
    ap.add_argument("--N", type=int, default=3)
    ap.add_argument("--solver", default="midpoint")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--precision", default="bf16", choices=["bf16", "fp32", "mixed", "bf16x3"])
    args = ap.parse_args()
    import flowdec_amd
    from flowdec_amd.dist import sharded_enhance
    dev = torch.device("cuda:0")
    model = flowdec_amd.from_preset("flow_model_sgmse", precision=args.precision)
    g = torch.Generator().manual_seed(0)
    sd = {}
    for k, v in model.state_dict().items():   # the weight recipe of bench.py
        if not k.startswith("backbone."):
            continue
        if k.endswith("all_modules.0.W"):
            sd[k] = torch.randn(v.shape, generator=g) * 16.0
        elif v.ndim == 1 and k.endswith("weight"):
            sd[k] = 1.0 + 0.1 * torch.randn(v.shape, generator=g)
        elif k.endswith("bias") or k.endswith(".b"):
            sd[k] = 0.05 * torch.randn(v.shape, generator=g)
        elif k.endswith(".W"):   # NIN [in, out]
            sd[k] = torch.randn(v.shape, generator=g) / v.shape[0] ** 0.5
        else:
            sd[k] = torch.randn(v.shape, generator=g) / v[0].numel() ** 0.5
    model.load_state_dict(sd, strict=False)
    model = model.to(dev)
    Lw = int(args.seconds * 48000)
    y = 0.1 * torch.randn(args.batch, 1, Lw, device=dev, generator=torch.Generator(device=dev).manual_seed(0))

    def step(k):
        return sharded_enhance(model, y, N=args.N, solver=args.solver, seed=1000 + k, use_graph=True)

    for k in range(args.warmup):
        step(k)
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for k in range(args.steps):
        out = step(k)
    torch.cuda.synchronize(dev)
    el = time.perf_counter() - t0
    nfe = {"euler": args.N, "midpoint": 2 * args.N}.get(args.solver, 2 * args.N)
    audio = args.batch * args.seconds * args.steps
    print(json.dumps({"metric": "sgmse_enhance_throughput", "value": audio / el, "unit": "audio-seconds/second", "preset": "flow_model_sgmse",
                      "batch": args.batch, "seconds": args.seconds, "solver": args.solver, "N": args.N, "nfe": nfe, "steps": args.steps,
                      "warmup": args.warmup, "ms_per_step": 1e3 * el / args.steps, "ms_per_nfe": 1e3 * el / args.steps / nfe,
                      "precision": args.precision, "graph": True, "finite": bool(torch.isfinite(out).all()),
                      "device": torch.cuda.get_device_name(dev)}))


if __name__ == "__main__":
    main()
