"""The validation loss of ONE set of pairs on ONE set of draws in the four precisions: the bf16 error on the objective the weights were
trained on, with no ODE solver in the way.  Every precision sees the same pairs, the same seeded noise and the same times (pair i is
seeded clip_seed(--seed, i); the library's noise does not depend on the precision), so the differences are the network's alone.

Default: synthetic pairs (a seeded "clean" signal and a perturbed "coded" one) on the seeded full-width weights of the 75m preset -- random
weights, so the numbers say how the modes differ on SOME network of that shape, not on a trained one.  --ckpt C (with --pairs-file P, the
list format of loss_cli) runs a real checkpoint on real pairs.

    python scripts/valid_loss_by_precision.py [--pairs 16] [--seconds 2] [--batch 8] [--seed 0] [--ckpt C --pairs-file P] [--out J]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PRECISIONS = ("fp32", "bf16x3", "mixed", "bf16")


def synthetic_pairs(n, seconds, seed=0):
    rng = np.random.default_rng(seed)
    L = int(seconds * 48000)
    xs, ys = [], []
    for _ in range(n):
        x = (0.1 * rng.standard_normal(L)).astype(np.float32)
        xs.append(torch.from_numpy(x))
        ys.append(torch.from_numpy((x + 0.03 * rng.standard_normal(L)).astype(np.float32)))
    return xs, ys


def seeded_model(precision, weight_seed=64):
    import flowdec_amd
    from oracle import flowdec_oracle as O
    m = flowdec_amd.from_preset("flowdec_75m", precision=precision)
    sd = {k: torch.from_numpy(v) for k, v in O.random_state_dict(seed=weight_seed, nf=64).items() if k.startswith("backbone.")}
    m.load_state_dict(sd, strict=False)
    return m.cuda()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=16)
    ap.add_argument("--seconds", type=float, default=2.0)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--ckpt", default=None)
    ap.add_argument("--pairs-file", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from flowdec_amd import loss_cli
    from flowdec_amd.checkpoint import load_from_checkpoint
    if args.ckpt:
        if not args.pairs_file:
            ap.error("--ckpt needs --pairs-file")
        la = loss_cli.build_parser().parse_args(["--ckpt", args.ckpt, "--pairs-file", args.pairs_file, "--target-duration", str(args.seconds)])
        _, xs, ys = loss_cli.load_pairs(la, 48000)
    else:
        xs, ys = synthetic_pairs(args.pairs, args.seconds)
    rows = {}
    for prec in PRECISIONS:
        m = load_from_checkpoint(args.ckpt, map_location="cuda", precision=prec) if args.ckpt else seeded_model(prec)
        kind = loss_cli.model_kind_of(m)
        kw = {} if kind == "regression" else dict(seeds=args.seed)
        rows[prec] = dict(loss=float(m.valid_loss_batch(xs, ys, max_batch=args.batch, **kw)), per_pair=[float(v) for v in m.last_loss_info["per_clip"]])
        del m
        torch.cuda.empty_cache()
    ref = rows["fp32"]
    for prec, r in rows.items():
        r["rel_diff_to_fp32"] = (r["loss"] - ref["loss"]) / ref["loss"]
        pp, pr = np.array(r["per_pair"]), np.array(ref["per_pair"])
        r["max_rel_diff_per_pair"] = float(np.abs(pp - pr).max() / np.abs(pr).max()) if len(pp) else 0.0
    out = dict(what="valid_loss by precision, same pairs / noise / times", weights=args.ckpt or "seeded flowdec_75m (random, seed 64)", kind=kind,
               pairs=len(xs), seconds=args.seconds, seed=args.seed, device=torch.cuda.get_device_name(0),
               rows={p: {k: v for k, v in r.items() if k != "per_pair"} for p, r in rows.items()})
    print("%-8s %-16s %-14s %s" % ("mode", "valid_loss", "rel. to fp32", "max per-pair diff / max per-pair loss"))
    for p in PRECISIONS:
        r = rows[p]
        print("%-8s %-16.8g %-+14.3e %.3e" % (p, r["loss"], r["rel_diff_to_fp32"], r["max_rel_diff_per_pair"]))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
