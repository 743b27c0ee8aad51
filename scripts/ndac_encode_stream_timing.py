#!/usr/bin/env python
"""Cost of the one-launch quantiser and of streaming / long-form NDAC encode, at DAC's published full width with the ndac-75 frame rate
(FULL_WIDTH of tests/test_hip_ndac.py; random weights).

  (a) RVQ: `fd_rvq_encode` (one rvq_step_kernel launch per quantiser, a copy of z and a memset in front) against `fd_rvq_encode_chain`
      (rvq_chain_kernel, one launch) on the same latent, D = 1024, 10 quantisers, at 8 clips x 150 frames and at 1 clip x (block 8 +
      halos) frames -- the window a streaming encoder quantises.  The two are timed INTERLEAVED in one process, warm: each round times
      `--inner` back-to-back calls of one, then of the other, between two device events; reported: the median over the rounds of the
      time per call, with the fastest and slowest round.  The outputs are checked for bit equality first.
  (b) Streaming: one clip of S seconds encoded in one `DAC.encode` call, through `EncodeStream` fed one block of frames per push at
      block_frames 1 and 8, and through `DAC.encode_long`, in the precisions "exact" and "mfma"; per path the median wall time over
      `--iters` passes (interleaved: every pass runs all paths) with the fastest and slowest pass, the real-time factor, for the
      streams the host time per push (synchronised after every push: what a caller waiting for the codes sees) and the recompute share
      the window arithmetic predicts, (block + halo_left + halo_right) / block.  Every path's codes are checked against the one-shot
      encode for bit equality first.
    python scripts/ndac_encode_stream_timing.py [--seconds 10] [--iters 5] [--rounds 15] [--inner 20] [--window-frames 256] [--rows-per-call 4]"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from flowdec_amd import _lib as L  # noqa: E402
from flowdec_amd.ndac import DAC  # noqa: E402
from flowdec_amd.ndac_stream import EncodeStream  # noqa: E402

FULL_WIDTH = dict(encoder_dim=64, encoder_rates=(2, 4, 8, 10), decoder_dim=1536, decoder_rates=(10, 8, 4, 2), n_codebooks=10, codebook_size=1024,
                  codebook_dim=8, sample_rate=48000)


def spread(xs, scale=1e3):
    return {"median": scale * statistics.median(xs), "min": scale * min(xs), "max": scale * max(xs), "n": len(xs)}


def rvq_timing(m, B, T, rounds, inner):
    lib, h = L.load(), m.handle()
    z = torch.randn(B, m.latent_dim, T, device="cuda")
    nq, cd = m.n_codebooks, m.codebook_dim
    out = {k: (torch.empty_like(z), torch.empty(B, nq, T, dtype=torch.int32, device="cuda"), torch.empty(B, nq * cd, T, device="cuda")) for k in ("steps", "chain")}
    ws = torch.empty(z.numel() * 4, dtype=torch.uint8, device="cuda")

    def steps():
        zq, codes, lat = out["steps"]
        L.check(lib.fd_rvq_encode(h, L.ptr(z), B, T, nq, L.ptr(zq), L.ptr(codes), L.ptr(lat), L.ptr(ws), ws.numel(), L.stream()))

    def chain():
        zq, codes, lat = out["chain"]
        L.check(lib.fd_rvq_encode_chain(h, L.ptr(z), None, B, T, nq, L.ptr(zq), L.ptr(codes), L.ptr(lat), L.stream()))

    steps(); chain(); torch.cuda.synchronize()
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(out["steps"], out["chain"])), "the chain kernel is not the step launches"
    times = {"steps": [], "chain": []}
    for _ in range(3):
        steps(); chain()
    for r in range(rounds):
        for name, fn in (("steps", steps), ("chain", chain)) if r % 2 == 0 else (("chain", chain), ("steps", steps)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(inner):
                fn()
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) / inner / 1e3)
    res = {"shape": f"{B} x {m.latent_dim} x {T}, {nq} quantisers", "workgroups_per_launch": B * ((T + 7) // 8),
           "steps_us": spread(times["steps"], 1e6), "chain_us": spread(times["chain"], 1e6)}
    res["chain_vs_steps"] = res["chain_us"]["median"] / res["steps_us"]["median"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--window-frames", type=int, default=256)
    ap.add_argument("--rows-per-call", type=int, default=4)
    ap.add_argument("--blocks", type=int, nargs="*", default=[1, 8], help="EncodeStream block sizes to time")
    ap.add_argument("--skip-streaming", action="store_true")
    a = ap.parse_args()
    torch.manual_seed(0)
    m = DAC(**FULL_WIDTH)
    for k, p in m.named_parameters():          # keep activations O(1): g = 0.8 ||v||
        if k.endswith("weight_g"):
            v = dict(m.named_parameters())[k[:-1] + "v"]
            p.data = 0.8 * v.data.pow(2).sum(dim=tuple(range(1, v.ndim)), keepdim=True).sqrt()
    m = m.cuda()
    hop = m.hop_length
    hl, hr = m.encode_halo()
    res = {"config": "DAC 64/(2,4,8,10)/1536/(10,8,4,2), 10 x 1024 x 8 codebooks @ 48 kHz", "encode_halo_frames": [hl, hr],
           "rvq": {"batch_8x150": rvq_timing(m, 8, 150, a.rounds, a.inner), "window_1x%d" % (8 + hl + hr): rvq_timing(m, 1, 8 + hl + hr, a.rounds, a.inner)}}
    if a.skip_streaming:
        print(json.dumps(res))
        return
    T = int(a.seconds * m.sample_rate) // hop
    audio_s = T * hop / m.sample_rate
    x = 0.3 * torch.randn(T * hop, device="cuda")
    res["streaming_clip"] = f"one clip of {audio_s:g} s = {T} frames"

    def ws_bytes(B, frames):
        return L.load().fd_ndac_workspace_bytes(m.handle(), B, frames * hop)

    for precision in ("exact", "mfma"):
        m.precision = precision
        per_push = {b: [] for b in a.blocks}
        sessions = {}

        def one_shot():
            return m.encode(x[None, None])[1][0]

        def stream(block):
            st, outs = EncodeStream(m, block_frames=block, rows_per_call=a.rows_per_call), []
            per_push[block].clear()
            for f in range(0, T, block):
                t0 = time.perf_counter()
                outs.append(st.push(x[f * hop:(f + block) * hop]))
                torch.cuda.synchronize()
                per_push[block].append(time.perf_counter() - t0)
            outs.append(st.flush())
            sessions[block] = st
            return torch.cat(outs, dim=1)

        paths = [("one_shot", one_shot)] + [(f"stream_block_{b}", (lambda b=b: stream(b))) for b in a.blocks]
        paths.append(("encode_long", lambda: m.encode_long(x[None, None], window_frames=a.window_frames, rows_per_call=a.rows_per_call)[1][0]))
        want = one_shot()
        for name, fn in paths:                                  # warm, and the bits first
            assert torch.equal(fn(), want), f"{precision} {name}: not the one-shot encode"
        torch.cuda.synchronize()
        wall = {name: [] for name, _ in paths}
        for _ in range(a.iters):
            for name, fn in paths:
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                wall[name].append(time.perf_counter() - t0)
        r = {}
        base = statistics.median(wall["one_shot"])
        for name, _ in paths:
            r[name] = {"ms": spread(wall[name]), "rtf": statistics.median(wall[name]) / audio_s, "vs_one_shot": statistics.median(wall[name]) / base}
        for b in a.blocks:
            steady = per_push[b][(hr + b - 1) // b + 1:] or per_push[b]
            r[f"stream_block_{b}"].update({"pushes": len(per_push[b]), "push_ms": spread(steady), "block_ms_of_audio": 1e3 * b * hop / m.sample_rate,
                                           "frames_encoded_per_frame": sessions[b].frames_encoded / T, "predicted_recompute_share": (b + hl + hr) / b,
                                           "delay_ms": 1e3 * sessions[b].delay_samples / m.sample_rate})
        blk = a.window_frames - hl - hr
        r["encode_long"].update({"window_frames": a.window_frames, "rows_per_call": a.rows_per_call, "predicted_recompute_share": a.window_frames / blk,
                                 "workspace_mib": ws_bytes(a.rows_per_call, a.window_frames) / 2 ** 20, "one_shot_workspace_mib": ws_bytes(1, T) / 2 ** 20})
        res[precision] = r
    print(json.dumps(res))


if __name__ == "__main__":
    main()
