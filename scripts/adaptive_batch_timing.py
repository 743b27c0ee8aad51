#!/usr/bin/env python
"""What per-clip step control of the adaptive solvers costs and saves, on BASELINE config 5's per-GPU shard (FlowDec-75m, 8 x 4 s,
t_span = linspace(0, 1, 33), dopri5, bf16x3, atol = rtol = 1e-3) and on a ragged corpus of 1-4 s clips (the lengths of
scripts/cli_corpus_rtf.py).  Three ways to run the same clips, in one process, alternated `--reps` times after a warm-up of every shape:

  (a) one clip per call              m.enhance(clip)                               -- what a batch of an adaptive solver had to be so far
  (b) one batch, per-clip control    m.enhance(y, step_control='clip')             -- the same bits as (a), clip for clip (checked here)
  (c) one batch, one controller      m.enhance(y)                                  -- for context only: it computes a DIFFERENT result

Reported per run: wall seconds (host clock around work that ends in a device synchronise), the evaluations of the network that ran,
per-clip NFE and rejected attempts, and for (b) the share of wasted evaluations, 1 - sum_b nfe_b / (B x evals): clips that are done
ride along until the slowest clip of their batch is.  -> profiles/r07_adaptive_batch_timing.json (--out)

    python scripts/adaptive_batch_timing.py [--clips 8] [--seconds 4] [--N 32] [--tol 1e-3] [--reps 2] [--corpus-files 16] [--batch 8]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_cfg5_dopri5 import build  # noqa: E402  (FlowDec-75m at full width, seeded random weights)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, time.perf_counter() - t0


def waste(nfe, evals):
    return 1.0 - float(sum(nfe)) / (len(nfe) * evals)


def shard(m, a, res):
    Lw = int(a.seconds * 48000)
    gen = torch.Generator(device="cuda").manual_seed(5)
    y = 0.1 * torch.randn(a.clips, 1, Lw, device="cuda", generator=gen)
    Tp = 64 * ((1 + Lw // 384 + 63) // 64)
    nz = torch.randn(a.clips, 1, 768, Tp, dtype=torch.complex64, device="cuda", generator=gen)
    kw = dict(N=a.N, solver=a.solver, atol=a.tol, rtol=a.tol)

    def one_by_one():
        outs, nfe = [], []
        for b in range(a.clips):
            outs.append(m.enhance(y[b:b + 1], noise=nz[b:b + 1], **kw))
            nfe.append(m.last_nfe)
        return torch.cat(outs), nfe

    # warm-up: both batch sizes, every kernel of the solve (N = 1 at a loose tolerance: a handful of evaluations)
    m.enhance(y[:1], noise=nz[:1], N=1, solver=a.solver, atol=0.1, rtol=0.1)
    m.enhance(y, noise=nz, N=1, solver=a.solver, atol=0.1, rtol=0.1, step_control="clip")
    m.enhance(y, noise=nz, N=1, solver=a.solver, atol=0.1, rtol=0.1)
    runs = {"a_one_clip_per_call": [], "b_batch_per_clip_control": [], "c_batch_one_controller": []}
    same = True
    for _ in range(a.reps):
        (wa, nfe_a), ta = timed(one_by_one)
        runs["a_one_clip_per_call"].append({"seconds": ta, "evals_of_one_clip": int(sum(nfe_a)), "nfe_per_clip": nfe_a})
        wb, tb = timed(lambda: m.enhance(y, noise=nz, step_control="clip", **kw))
        nfe_b, rej_b = m.last_nfe_per_clip.tolist(), m.last_rejected_per_clip.tolist()
        runs["b_batch_per_clip_control"].append({"seconds": tb, "evals_of_the_batch": m.last_evals, "nfe_per_clip": nfe_b, "rejected_per_clip": rej_b,
                                                 "wasted_share": waste(nfe_b, m.last_evals)})
        same = same and torch.equal(wa, wb) and nfe_a == nfe_b
        wc, tc = timed(lambda: m.enhance(y, noise=nz, **kw))
        runs["c_batch_one_controller"].append({"seconds": tc, "evals_of_the_batch": m.last_nfe,
                                               "rel_l2_to_per_clip_result": float((wc - wb).norm() / wb.norm())})
        print(f"shard: (a) {ta:.2f} s, nfe {nfe_a} | (b) {tb:.2f} s, evals {runs['b_batch_per_clip_control'][-1]['evals_of_the_batch']}, rejected {rej_b} | "
              f"(c) {tc:.2f} s, nfe {runs['c_batch_one_controller'][-1]['evals_of_the_batch']} | (b) == (a): {same}", flush=True)
    res["shard"] = {"config": f"{a.clips} x {a.seconds:g} s, {a.solver} over linspace(0, 1, {a.N + 1}), atol = rtol = {a.tol:g}, {a.precision}",
                    "runs": runs, "b_bit_identical_to_a": same,
                    "b_over_a_seconds": [rb["seconds"] / ra["seconds"] for ra, rb in zip(runs["a_one_clip_per_call"], runs["b_batch_per_clip_control"])]}


def corpus(m, a, res):
    """1-4 s clips, bucketed by T_pad, `--batch` per call: (a) one by one against (b) enhance_batch(step_control='clip'), the library's seeds."""
    from flowdec_amd.model import padded_frames_of
    from flowdec_amd.noise import clip_seed
    rng = np.random.default_rng(0)
    lens = rng.integers(48000, 4 * 48000 + 1, size=a.corpus_files)
    clips = [torch.from_numpy((0.1 * rng.standard_normal(int(n))).astype(np.float32)).cuda() for n in lens]
    buckets = {}
    for i, n in enumerate(lens):
        buckets.setdefault(padded_frames_of(int(n)), []).append(i)
    batches = [idx[i:i + a.batch] for _, idx in sorted(buckets.items()) for i in range(0, len(idx), a.batch)]
    kw = dict(N=a.N, solver=a.solver, atol=a.tol, rtol=a.tol)
    seeds = [clip_seed(5, i) for i in range(len(clips))]
    for idx in batches:     # warm-up of every (B, T_pad) the timed window uses
        m.enhance(clips[idx[0]], seed=[seeds[idx[0]]], N=1, solver=a.solver, atol=0.1, rtol=0.1)
        m.enhance_batch([clips[i] for i in idx], seeds=[seeds[i] for i in idx], N=1, solver=a.solver, atol=0.1, rtol=0.1, step_control="clip")

    def one_by_one():
        out = {}
        for idx in batches:
            for i in idx:
                out[i] = (m.enhance(clips[i], seed=[seeds[i]], **kw), m.last_nfe)
        return out

    def batched():
        out, evals = {}, []
        for idx in batches:
            ws = m.enhance_batch([clips[i] for i in idx], seeds=[seeds[i] for i in idx], step_control="clip", **kw)
            for j, i in enumerate(idx):
                out[i] = (ws[j], int(m.last_nfe_per_clip[j]))
            evals.append((len(idx), m.last_evals))
        return out, evals

    rows = []
    for _ in range(a.reps):
        oa, ta = timed(one_by_one)
        (ob, evals), tb = timed(batched)
        same = all(torch.equal(oa[i][0], ob[i][0]) and oa[i][1] == ob[i][1] for i in oa)
        used, ran = sum(v[1] for v in ob.values()), sum(B * e for B, e in evals)
        rows.append({"a_seconds": ta, "b_seconds": tb, "b_over_a": tb / ta, "b_bit_identical_to_a": same, "sum_nfe_per_clip": used,
                     "clip_evaluations_run_by_b": ran, "wasted_share": 1.0 - used / ran})
        print(f"corpus: (a) {ta:.2f} s | (b) {tb:.2f} s | wasted share {1.0 - used / ran:.3f} | (b) == (a): {same}", flush=True)
    res["corpus"] = {"files": int(a.corpus_files), "audio_seconds": float(lens.sum()) / 48000, "batch": a.batch,
                     "batches": [[len(idx), int(padded_frames_of(int(lens[idx[0]])))] for idx in batches], "nfe_per_clip": [ob[i][1] for i in sorted(ob)],
                     "runs": rows}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=8)
    ap.add_argument("--seconds", type=float, default=4.0)
    ap.add_argument("--N", type=int, default=32)
    ap.add_argument("--tol", type=float, default=1e-3)
    ap.add_argument("--solver", default="dopri5", choices=["dopri5", "tsit5"])
    ap.add_argument("--precision", default="bf16x3", choices=["bf16", "bf16x3", "fp32", "mixed"])
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--corpus-files", type=int, default=16)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r07_adaptive_batch_timing.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("adaptive_batch_timing.py measures on the GPU: no device found")
    m = build(a.precision)
    res = {}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    shard(m, a, res)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    if a.corpus_files > 0:
        corpus(m, a, res)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
