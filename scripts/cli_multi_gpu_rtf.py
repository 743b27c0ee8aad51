#!/usr/bin/env python
"""`enhance_cli --gpus 1` against `enhance_cli --gpus G` on the synthetic corpus of scripts/cli_corpus_rtf.py (default 64 files, 1-4 s,
48 kHz, a full-width synthetic Lightning checkpoint, Euler-6, `--rng native --seed 5 --rtf`).  G is the device count of the box.  On a
one-GPU box the second run is `--gpus 2 --share-gpu`: two workers that SHARE the GPU, which can show what the launcher costs (process
start-up, a second checkpoint load, the merge) and nothing about a gain -- the JSON says so in `what_this_shows`.

Both runs are fresh `python -m flowdec_amd.enhance_cli` processes, so both wall clocks include interpreter start-up, the checkpoint load
and the graph capture of every (B, T_pad) bucket: that is what a user of the command line waits for.  GPU seconds are the `--rtf` sums
(over the ranks for --gpus G).  Every output file and the path column of rtfs.csv are compared byte for byte.

    python scripts/cli_multi_gpu_rtf.py [--files 64] [--N 6] [--solver euler] [--batch-files 8] [--out profiles/cli_multi_gpu_rtf.json]
"""
import argparse
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def run_cli(argv):
    """One fresh CLI process -> (wall seconds, audio seconds, GPU seconds of its aggregate `total:` line, stdout)."""
    env = dict(os.environ, PYTHONPATH=ROOT + (os.pathsep + os.environ["PYTHONPATH"] if os.environ.get("PYTHONPATH") else ""))
    t0 = time.perf_counter()
    r = subprocess.run([sys.executable, "-m", "flowdec_amd.enhance_cli"] + argv, env=env, capture_output=True, text=True)
    wall = time.perf_counter() - t0
    if r.returncode != 0:
        raise RuntimeError(f"enhance_cli exited with {r.returncode}:\n" + (r.stdout + r.stderr)[-3000:])
    m = [re.match(r"total: ([0-9.]+) s of audio in ([0-9.]+) s of GPU time", ln) for ln in r.stdout.splitlines()]
    m = [x for x in m if x]
    assert len(m) == 1, r.stdout[-2000:]
    return wall, float(m[0].group(1)), float(m[0].group(2)), r.stdout


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=64)
    ap.add_argument("--min-s", type=float, default=1.0)
    ap.add_argument("--max-s", type=float, default=4.0)
    ap.add_argument("--N", type=int, default=6)
    ap.add_argument("--solver", default="euler")
    ap.add_argument("--batch-files", type=int, default=8)
    ap.add_argument("--precision", default="bf16", choices=["bf16", "fp32", "bf16x3", "mixed"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cli_multi_gpu_rtf.json"))
    args = ap.parse_args()
    import flowdec_amd
    from flowdec_amd import audio, enhance_cli

    tmp = tempfile.mkdtemp(prefix="fd_multi_")
    try:
        # the checkpoint and the corpus of scripts/cli_corpus_rtf.py: full-width FlowDec-75m, seeded random weights, Lightning layout
        m = flowdec_amd.from_preset("flowdec_75m", precision=args.precision)
        g = torch.Generator().manual_seed(1234)
        sd = {}
        for k, v in m.state_dict().items():
            if k.endswith(".W"):
                sd[k] = torch.randn(v.shape, generator=g) * 16.0
            elif k.startswith("backbone.") and v.ndim == 1 and k.endswith("weight"):
                sd[k] = 1.0 + 0.1 * torch.randn(v.shape, generator=g)
            elif k.startswith("backbone.") and k.endswith("bias"):
                sd[k] = 0.05 * torch.randn(v.shape, generator=g)
            elif k.startswith("backbone."):
                sd[k] = torch.randn(v.shape, generator=g) / v[0].numel() ** 0.5
            else:
                sd[k] = v.clone()
        ckpt = os.path.join(tmp, "flowdec_75m_synthetic.ckpt")
        torch.save({"_pl_ema_state_dict": sd, "state_dict": sd}, ckpt)
        ind = os.path.join(tmp, "in")
        os.makedirs(ind)
        rng = np.random.default_rng(0)
        lens = rng.integers(int(args.min_s * 48000), int(args.max_s * 48000) + 1, size=args.files)
        for i, n in enumerate(lens):
            audio.save_wav(os.path.join(ind, f"clip{i:03d}.wav"), torch.from_numpy((0.1 * rng.standard_normal((1, int(n)))).astype(np.float32)), 48000)
        devices = enhance_cli.visible_gpus()
        if devices < 1:
            raise RuntimeError("no GPU visible")
        shared = devices == 1
        world = 2 if shared else devices
        common = ["--ckpt", ckpt, "--files", ind, "--N", str(args.N), "--solver", args.solver, "--rtf", "--rng", "native", "--seed", "5",
                  "--batch-files", str(args.batch_files), "--precision", args.precision]
        res = {"files": int(args.files), "audio_seconds": float(lens.sum()) / 48000, "lengths_s": [args.min_s, args.max_s], "N": args.N,
               "solver": args.solver, "precision": args.precision, "batch_files": args.batch_files, "visible_gpus": devices, "runs": {}}
        outs = {}
        for name, extra in (("gpus_1", ["--gpus", "1"]), (f"gpus_{world}" + ("_share_gpu" if shared else ""),
                                                          ["--gpus", str(world)] + (["--share-gpu"] if shared else []))):
            outs[name] = os.path.join(tmp, name)
            wall, audio, gpu_s, stdout = run_cli(common + extra + ["--outdir", outs[name]])
            per_rank = [int(x) for x in re.findall(r"worker \d+ of \d+ on \S+ (\d+) of \d+ batches", stdout)]
            res["runs"][name] = {"wall_seconds_whole_process": wall, "gpu_seconds_summed_over_ranks": gpu_s, "audio_seconds": audio,
                                 "audio_seconds_per_wall_second": audio / wall, "audio_seconds_per_gpu_second": audio / gpu_s,
                                 "batches_per_rank": per_rank}
            print(f"{name}: {audio:.1f} s of audio, wall {wall:.2f} s ({audio / wall:.1f} x real time), GPU {gpu_s:.3f} s summed "
                  f"({audio / gpu_s:.1f} x)", flush=True)
        a, b = outs.values()
        names = sorted(os.listdir(ind))
        res["outputs_identical"] = all(open(os.path.join(a, f), "rb").read() == open(os.path.join(b, f), "rb").read() for f in names)
        rows = [[ln.split(",")[0].split("/")[-1] for ln in open(os.path.join(d, "rtfs.csv")).read().splitlines()[1:]] for d in (a, b)]
        res["rtfs_paths_identical"] = rows[0] == rows[1] and len(rows[0]) == len(names)
        res["directory_listings_identical"] = sorted(os.listdir(a)) == sorted(os.listdir(b))
        res["what_this_shows"] = ("two workers SHARING the one GPU of this box: the launcher's overhead (start-up, a second checkpoint load, the merge) "
                                  "and byte identity only -- the multi-GPU rate is unmeasured" if shared else
                                  f"{world} workers on {world} GPUs against one process on one GPU, whole-process wall clock")
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
        print(json.dumps(res))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
