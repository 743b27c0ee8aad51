#!/usr/bin/env python
"""Cost of a codec pool step against the same sessions as independent streams, at DAC's published full width with the ndac-75 frame rate
(the codec of scripts/ndac_stream_timing.py; random weights), in both directions.

One STEP gives each of S sessions one block of input and runs everything that became ready; its wall time is taken with one device
synchronisation at its end (what a server that waits for all its sessions' outputs sees).  Three paths, interleaved repetition by repetition:

  * streams     S independent `DecodeStream` / `EncodeStream` sessions pushed round-robin in the same process: the yardstick
  * pool        one `DecodePool` / `EncodePool` with S sessions, use_graph=False: one native call per step
  * pool_graph  the same with use_graph=True: one graph replay per step

Only steady steps are timed (every window at its full length).  Before any timing every path's concatenated output, flush included, is
compared with the one-shot decode / encode of each session for bit equality.  Reported per (direction, S, block, path): the median step
(and the median of the host's share of it: the time until everything was enqueued) over all timed steps of a repetition, then median /
minimum / maximum over the repetitions, and the sessions one GPU carries at real time, S * (block duration) / (step time).
    python scripts/ndac_pool_timing.py [--sessions 1 8 32] [--blocks 1 8] [--steps 20] [--reps 3] [--precision mfma_decoder] [--out FILE.json]"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from flowdec_amd.ndac import DAC  # noqa: E402
from flowdec_amd.ndac_pool import DecodePool, EncodePool  # noqa: E402
from flowdec_amd.ndac_stream import DecodeStream, EncodeStream  # noqa: E402

FULL_WIDTH = dict(encoder_dim=64, encoder_rates=(2, 4, 8, 10), decoder_dim=1536, decoder_rates=(10, 8, 4, 2), n_codebooks=10, codebook_size=1024,
                  codebook_dim=8, sample_rate=48000)
PATHS = ("streams", "pool", "pool_graph")


def build(precision):
    torch.manual_seed(0)
    m = DAC(**FULL_WIDTH, precision=precision)
    for k, p in m.named_parameters():          # keep activations O(1): g = 0.8 ||v||
        if k.endswith("weight_g"):
            v = dict(m.named_parameters())[k[:-1] + "v"]
            p.data = 0.8 * v.data.pow(2).sum(dim=tuple(range(1, v.ndim)), keepdim=True).sqrt()
    return m.cuda()


class Streams:
    """S independent stream sessions behind the pools' push / step / flush shape."""

    def __init__(self, make):
        self.make, self.st, self.got = make, [], {}

    def open(self, nq):
        self.st.append(self.make(nq))
        return len(self.st) - 1

    def push(self, sid, x):
        self.got[sid] = self.st[sid].push(x)

    def step(self):
        got, self.got = self.got, {}
        return got

    def flush(self, sid):
        return self.st[sid].flush()


def run(direction, path, pools, m, inputs, block, n_steps, timed_from):
    """All sessions through `n_steps` steps of one block each, then flushed -> (per-session concatenated output, [seconds of the timed steps],
    [the host's share of each: until everything was enqueued])."""
    unit = block * (m.hop_length if direction == "encode" else 1)
    nq = m.n_codebooks
    if path == "streams":
        cls = EncodeStream if direction == "encode" else DecodeStream
        pool = Streams(lambda q: cls(m, n_quantizers=q, block_frames=block))
    else:
        pool = pools[path]
    sids = [pool.open(nq) for _ in inputs]
    outs, times, enq = [[] for _ in inputs], [], []
    for i in range(n_steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for sid, x in zip(sids, inputs):
            pool.push(sid, x[..., i * unit:(i + 1) * unit])
        got = pool.step()
        t1 = time.perf_counter()
        torch.cuda.synchronize()
        if i >= timed_from:
            times.append(time.perf_counter() - t0)
            enq.append(t1 - t0)
        for k, sid in enumerate(sids):
            if sid in got:
                outs[k].append(got[sid])
    for k, sid in enumerate(sids):
        outs[k].append(pool.flush(sid))
    return [torch.cat(o, dim=-1) for o in outs], times, enq


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sessions", type=int, nargs="*", default=[1, 8, 32])
    ap.add_argument("--blocks", type=int, nargs="*", default=[1, 8])
    ap.add_argument("--steps", type=int, default=20, help="timed steps per repetition")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--precision", default="mfma_decoder", help="DAC.precision: the decoder's / the encoder's arithmetic")
    ap.add_argument("--directions", nargs="*", default=["decode", "encode"])
    ap.add_argument("--out", default=None, help="also write the result lines to this JSON file")
    a = ap.parse_args()
    m = build(a.precision)
    hop, sr = m.hop_length, m.sample_rate
    lines = []
    for direction in a.directions:
        hl, hr = m.encode_halo() if direction == "encode" else m.decode_halo()
        for block in a.blocks:
            warm = -(-(hl + hr) // block) + 2               # steps until every window has its full length
            n_steps = warm + a.steps
            for S in a.sessions:
                g = torch.Generator().manual_seed(1000 * S + block)
                if direction == "encode":
                    inputs = [0.3 * torch.randn(n_steps * block * hop, generator=g) for _ in range(S)]
                    want = [m.encode(x[None, None].cuda())[1][0] for x in inputs]
                else:
                    inputs = [torch.randint(0, m.codebook_size, (m.n_codebooks, n_steps * block), generator=g) for _ in range(S)]
                    want = [m.decode(m.quantizer.from_codes(c[None].cuda())[0])[0, 0] for c in inputs]
                cls = EncodePool if direction == "encode" else DecodePool
                pools = {"pool": cls(m, capacity=S, block_frames=block, use_graph=False), "pool_graph": cls(m, capacity=S, block_frames=block, use_graph=True)}
                for path in PATHS:                           # bit equality first (and the warm-up: the graph is captured here)
                    got = run(direction, path, pools, m, inputs, block, n_steps, warm)[0]
                    for k in range(S):
                        assert torch.equal(got[k], want[k]), f"{direction} S={S} block={block} {path}: session {k} is not its one-shot result"
                per_rep, per_rep_enq = {p: [] for p in PATHS}, {p: [] for p in PATHS}
                for _ in range(a.reps):                      # interleaved: one repetition of each path in turn
                    for path in PATHS:
                        _, times, enq = run(direction, path, pools, m, inputs, block, n_steps, warm)
                        per_rep[path].append(1e3 * statistics.median(times))
                        per_rep_enq[path].append(1e3 * statistics.median(enq))
                block_ms = 1e3 * block * hop / sr
                for path in PATHS:
                    med = statistics.median(per_rep[path])
                    lines.append({"direction": direction, "precision": a.precision, "S": S, "block": block, "path": path, "step_ms": med,
                                  "step_ms_min": min(per_rep[path]), "step_ms_max": max(per_rep[path]), "enqueue_ms": statistics.median(per_rep_enq[path]), "sessions_at_real_time": S * block_ms / med,
                                  "vs_streams": med / statistics.median(per_rep["streams"]), "timed_steps": a.steps, "reps": a.reps,
                                  "native_calls_per_step": 1 if path != "streams" else None})
                    print(json.dumps(lines[-1]), flush=True)
    print("\n| direction | S | block | path | step ms (min .. max) | host enqueue ms | vs streams | sessions / GPU at real time |\n|---|---|---|---|---|---|---|---|")
    for r in lines:
        print(f"| {r['direction']} | {r['S']} | {r['block']} | {r['path']} | {r['step_ms']:.2f} ({r['step_ms_min']:.2f} .. {r['step_ms_max']:.2f}) | {r['enqueue_ms']:.2f} | "
              f"{r['vs_streams']:.2f} | {r['sessions_at_real_time']:.1f} |")
    if a.out:
        with open(a.out, "w") as f:
            json.dump({"config": f"DAC 64/(2,4,8,10)/1536/(10,8,4,2), 10 x 1024 x 8 codebooks @ 48 kHz, precision {a.precision}", "lines": lines}, f, indent=1)


if __name__ == "__main__":
    main()
