#!/usr/bin/env python
"""What the device driver of the ScoreDec ODE sampler costs against the host driver, and what batching under per-clip step control
costs and saves: `baseline_scoredec_75s` at full width (seeded random weights, the output layer scaled by --out-scale so that the
probability-flow ODE of an untrained network stays tame), rtol = atol = --tol (default 1e-3), in fp32 and bf16x3.  Per precision, in ONE
process, the arms alternated `--reps` times after a warm-up of every shape:

  one 2 s clip        (h) enhance(sampler_type='ode')                    scipy on the host around fd_score_eval
                      (d) enhance(sampler_type='ode', driver='device')   one native call
  eight clips, 1-4 s  (a) one clip per call, driver='device'
                      (b) enhance_ode_batch, bucketed by T_pad           the same bits as (a), clip for clip (checked here)

Reported: wall seconds (host clock around work that ends in a device synchronise), NFE, the waveform distance of (d) to (h), per-clip
NFE, and for (b) the share of evaluations wasted on clips that ride along, 1 - sum_b nfe_b / sum_batches (B x evals).  Then bf16 and mixed
run the 2 s clip once each on the device driver: finite audio, or the library's error.  -> profiles/score_ode_timing.json (--out)

    python scripts/score_ode_timing.py [--tol 1e-3] [--reps 3] [--out-scale 0.05] [--precisions fp32,bf16x3]
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
import flowdec_amd  # noqa: E402
from flowdec_amd.batching import padded_frames_of  # noqa: E402
from flowdec_amd.noise import clip_seed  # noqa: E402


def build(precision, out_scale):
    m = flowdec_amd.from_preset("baseline_scoredec_75s", precision=precision)
    g = torch.Generator().manual_seed(1234)
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
    sd["backbone.output_layer.weight"] = sd["backbone.output_layer.weight"] * out_scale
    m.load_state_dict(sd, strict=False)
    return m.cuda()


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, time.perf_counter() - t0


def one_clip(m, a, rng):
    y = torch.from_numpy((0.1 * rng.standard_normal(2 * 48000)).astype(np.float32)).cuda()
    kw = dict(sampler_type="ode", N=30, rtol=a.tol, atol=a.tol, seed=[clip_seed(5, 0)], return_nfe=True)
    m.enhance(y, driver="device", **dict(kw, rtol=0.1, atol=0.1))      # warm-up of both drivers' kernels and buffers
    m.enhance(y, **dict(kw, rtol=0.1, atol=0.1))
    rows = []
    for _ in range(a.reps):
        (xh, nh), th = timed(lambda: m.enhance(y, **kw))
        (xd, nd), td = timed(lambda: m.enhance(y, driver="device", **kw))
        rows.append({"host_seconds": th, "device_seconds": td, "host_over_device": th / td, "nfe_host": nh, "nfe_device": nd,
                     "device_vs_host_rel_l2": float((xd - xh).norm() / xh.norm())})
        print(f"  2 s clip: host {th:.3f} s (nfe {nh}) | device {td:.3f} s (nfe {nd}) | rel l2 {rows[-1]['device_vs_host_rel_l2']:.2e}", flush=True)
    return rows


def eight_clips(m, a, rng):
    lens = rng.integers(48000, 4 * 48000 + 1, size=8)
    clips = [torch.from_numpy((0.1 * rng.standard_normal(int(n))).astype(np.float32)).cuda() for n in lens]
    seeds = [clip_seed(5, i) for i in range(8)]
    buckets = {}
    for i, n in enumerate(lens):
        buckets.setdefault(padded_frames_of(int(n), 384), []).append(i)
    batches = [idx for _, idx in sorted(buckets.items())]
    kw = dict(N=30, rtol=a.tol, atol=a.tol)
    for idx in batches:     # warm-up of every (B, T_pad) the timed window uses
        m.enhance(clips[idx[0]], sampler_type="ode", driver="device", N=30, rtol=0.1, atol=0.1, seed=[seeds[idx[0]]])
        m.enhance_ode_batch([clips[i] for i in idx], N=30, rtol=0.1, atol=0.1, seeds=[seeds[i] for i in idx])

    def one_by_one():
        return {i: m.enhance(clips[i], sampler_type="ode", driver="device", seed=[seeds[i]], return_nfe=True, **kw) for idx in batches for i in idx}

    def batched():
        out, evals = {}, []
        for idx in batches:
            ws, nfe = m.enhance_ode_batch([clips[i] for i in idx], seeds=[seeds[i] for i in idx], return_nfe=True, **kw)
            out.update({i: (ws[j], nfe[j]) for j, i in enumerate(idx)})
            evals.append((len(idx), m.last_evals))
        return out, evals

    rows = []
    for _ in range(a.reps):
        oa, ta = timed(one_by_one)
        (ob, evals), tb = timed(batched)
        same = all(torch.equal(oa[i][0], ob[i][0]) and oa[i][1] == ob[i][1] for i in oa)
        used, ran = sum(v[1] for v in ob.values()), sum(B * e for B, e in evals)
        rows.append({"a_seconds": ta, "b_seconds": tb, "b_over_a": tb / ta, "b_bit_identical_to_a": same, "nfe_per_clip": [ob[i][1] for i in sorted(ob)],
                     "sum_nfe_per_clip": used, "clip_evaluations_run_by_b": ran, "wasted_share": 1.0 - used / ran})
        print(f"  8 clips: (a) {ta:.3f} s | (b) {tb:.3f} s | nfe {rows[-1]['nfe_per_clip']} | wasted {rows[-1]['wasted_share']:.3f} | (b) == (a): {same}",
              flush=True)
    return {"audio_seconds": float(lens.sum()) / 48000, "batches": [[len(idx), int(padded_frames_of(int(lens[idx[0]]), 384))] for idx in batches],
            "runs": rows}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tol", type=float, default=1e-3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out-scale", type=float, default=0.05)
    ap.add_argument("--precisions", default="fp32,bf16x3")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "score_ode_timing.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("score_ode_timing.py measures on the GPU: no device found")
    res = {"config": f"baseline_scoredec_75s, random weights (output layer x {a.out_scale:g}), RK45 rule, rtol = atol = {a.tol:g}, N = 30, denoise", "runs": {}}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    for prec in a.precisions.split(","):
        print(prec, flush=True)
        m = build(prec, a.out_scale)
        rng = np.random.default_rng(0)
        res["runs"][prec] = {"one_clip_2s": one_clip(m, a, rng), "eight_clips_1_4s": eight_clips(m, a, rng)}
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
        del m
        torch.cuda.empty_cache()
    res["low_precision"] = {}
    for prec in ("bf16", "mixed"):      # must run: finite audio, or the library's own error
        m = build(prec, a.out_scale)
        y = torch.from_numpy((0.1 * np.random.default_rng(0).standard_normal(2 * 48000)).astype(np.float32)).cuda()
        try:
            (x, nfe), dt = timed(lambda: m.enhance(y, sampler_type="ode", driver="device", N=30, rtol=a.tol, atol=a.tol, seed=[clip_seed(5, 0)],
                                                   return_nfe=True))
            res["low_precision"][prec] = {"seconds": dt, "nfe": nfe, "finite": bool(torch.isfinite(x).all())}
        except RuntimeError as e:
            res["low_precision"][prec] = {"error": str(e)}
        print(prec, res["low_precision"][prec], flush=True)
        del m
        torch.cuda.empty_cache()
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
