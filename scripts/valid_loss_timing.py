"""Timing of FlowModel.valid_loss_batch (one fused native call per batch: pair front end, state kernel, one network evaluation, float64
reduction) against THE SAME COMPUTATION COMPOSED FROM THE PUBLIC CALLS THAT EXISTED BEFORE IT -- `model._preprocess(y, x=x)`, torch
operations on the device for the draws, Xt, Ut and the squared error, and `model(xt, Y, t)` for the network.  That composition is what a
user could write without valid_loss_batch; it is labelled "composed" below.  Both sides see the same synthetic pairs (host tensors: both
include their host-to-device copies), run interleaved in one process, `--repeats` times each after one warm-up, and are reported in pairs
per second.  The composed side draws its noise with torch.randn (its values differ from the fused side's; the cost does not).

    python scripts/valid_loss_timing.py [--pairs 64] [--seconds 2] [--batch 8] [--precision bf16] [--repeats 3] [--out J]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def composed_loss(m, xs, ys, batch):
    """FlowModel._loss (model.py:421-468) from public calls and torch ops, in batches of `batch` pairs of one length."""
    per = []
    for i in range(0, len(xs), batch):
        x = torch.stack(xs[i:i + batch]).unsqueeze(1)
        y = torch.stack(ys[i:i + batch]).unsqueeze(1)
        Y, X, _ = m._preprocess(y, x=x)
        t = torch.rand(Y.shape[0], device=Y.device)
        Ys = Y + (m.sigma_y.to(Y.device) * torch.randn_like(Y)).type(Y.dtype)
        Xs = X if float(m.sigma_x) == 0 else X + (m.sigma_x * torch.randn_like(X)).type(X.dtype)
        tb = t[:, None, None, None]
        Xt, Ut = tb * Xs + (1 - tb) * Ys, Xs - Ys
        V = m(Xt, Y, t)
        per.append(((V - Ut).abs() ** 2).flatten(start_dim=1).mean(dim=1))
    return float(torch.cat(per).mean())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=64)
    ap.add_argument("--seconds", type=float, default=2.0)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--precision", default="bf16")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from valid_loss_by_precision import seeded_model, synthetic_pairs
    xs, ys = synthetic_pairs(args.pairs, args.seconds)
    m = seeded_model(args.precision)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        v = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, v

    fused = lambda: m.valid_loss_batch(xs, ys, seeds=0, max_batch=args.batch)
    composed = lambda: composed_loss(m, xs, ys, args.batch)
    timed(fused); timed(composed)          # warm-up: weights packed, workspaces allocated
    fs, cs = [], []
    for _ in range(args.repeats):
        s, vf = timed(fused); fs.append(s)
        s, vc = timed(composed); cs.append(s)
    f, c = statistics.median(fs), statistics.median(cs)
    # where the time goes: the network evaluations alone, on device-resident inputs of one batch, as often as either side runs them
    Y, X, _ = m._preprocess(torch.stack(ys[:args.batch]).unsqueeze(1), x=torch.stack(xs[:args.batch]).unsqueeze(1))
    tt = torch.rand(Y.shape[0], device=Y.device)
    n_calls = (args.pairs + args.batch - 1) // args.batch
    net_s = statistics.median(timed(lambda: [m(X, Y, tt) for _ in range(n_calls)])[0] for _ in range(args.repeats))
    out = dict(what="valid_loss of %d synthetic pairs of %.1f s, flowdec_75m seeded weights, %s, batches of %d" % (args.pairs, args.seconds, args.precision, args.batch),
               device=torch.cuda.get_device_name(0), fused_seconds=fs, composed_seconds=cs, fused_pairs_per_s=args.pairs / f,
               composed_from_public_calls_pairs_per_s=args.pairs / c, ratio_composed_over_fused=c / f, fused_loss=vf, composed_loss=vc,
               network_only_seconds=net_s, network_share_of_fused=net_s / f, network_share_of_composed=net_s / c)
    print("fused valid_loss_batch          : %.1f pairs/s" % (args.pairs / f))
    print("composed from public calls+torch: %.1f pairs/s" % (args.pairs / c))
    print("network evaluations alone       : %.3f s of %.3f s (fused) / %.3f s (composed)" % (net_s, f, c))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fo:
            json.dump(out, fo, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
