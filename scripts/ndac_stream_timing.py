#!/usr/bin/env python
"""Cost of streaming and long-form NDAC decode against the one-shot decode, at DAC's published full width with the ndac-75 frame rate
(FULL_WIDTH of tests/test_hip_ndac.py; random weights): one clip of S seconds of codes decoded

  * in one `DAC.decode` call (with `quantizer.from_codes` in front, as the streaming paths run it),
  * through `DecodeStream` fed one block of frames per push at block_frames 1 / 4 / 16 / 64,
  * through `DAC.decode_long` at the given window.

Reported per path: wall time, real-time factor (compute seconds per audio second), for the streams the host time per push (mean and
worst, synchronised after every push: what a caller waiting for the samples sees) and the recompute share the window arithmetic predicts,
(block + halo_left + halo_right) / block.  Every path's output is checked against the one-shot decode for bit equality first.
    python scripts/ndac_stream_timing.py [--seconds 20] [--iters 3] [--window-frames 256] [--rows-per-call 4] [--blocks 1 4 16 64]"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from flowdec_amd import _lib as L  # noqa: E402
from flowdec_amd.ndac import DAC  # noqa: E402
from flowdec_amd.ndac_stream import DecodeStream  # noqa: E402

FULL_WIDTH = dict(encoder_dim=64, encoder_rates=(2, 4, 8, 10), decoder_dim=1536, decoder_rates=(10, 8, 4, 2), n_codebooks=10, codebook_size=1024,
                  codebook_dim=8, sample_rate=48000)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=20.0)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--window-frames", type=int, default=256)
    ap.add_argument("--rows-per-call", type=int, default=4)
    ap.add_argument("--blocks", type=int, nargs="*", default=[1, 4, 16, 64], help="DecodeStream block sizes to time")
    a = ap.parse_args()
    torch.manual_seed(0)
    m = DAC(**FULL_WIDTH)
    for k, p in m.named_parameters():          # keep activations O(1): g = 0.8 ||v||
        if k.endswith("weight_g"):
            v = dict(m.named_parameters())[k[:-1] + "v"]
            p.data = 0.8 * v.data.pow(2).sum(dim=tuple(range(1, v.ndim)), keepdim=True).sqrt()
    m = m.cuda()
    T = int(a.seconds * m.sample_rate) // m.hop_length
    audio_s = T * m.hop_length / m.sample_rate
    codes = torch.randint(0, m.codebook_size, (m.n_codebooks, T), device="cuda")
    hl, hr = m.decode_halo()

    def ws_bytes(B, frames):
        return L.load().fd_ndac_workspace_bytes(m.handle(), B, frames * m.hop_length)

    def one_shot():
        return m.decode(m.quantizer.from_codes(codes[None])[0])[0, 0]

    def timed(fn):
        fn(); torch.cuda.synchronize()
        best = float("inf")
        for _ in range(a.iters):
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            best = min(best, time.perf_counter() - t0)
        return best, out

    res = {"config": f"DAC 64/(2,4,8,10)/1536/(10,8,4,2), 10 x 1024 x 8 codebooks, one clip of {audio_s:g} s = {T} frames @ 48 kHz, precision {m.precision}",
           "halo_frames": [hl, hr], "iters": a.iters}
    dt, want = timed(one_shot)
    res["one_shot"] = {"ms": 1e3 * dt, "rtf": dt / audio_s}
    for block in a.blocks:
        per_push = []

        def stream():
            st, outs = DecodeStream(m, block_frames=block, rows_per_call=a.rows_per_call), []
            per_push.clear()
            for f in range(0, T, block):
                t0 = time.perf_counter()
                outs.append(st.push(codes[:, f:f + block]))
                torch.cuda.synchronize()
                per_push.append(time.perf_counter() - t0)
            outs.append(st.flush())
            stream.st = st
            return torch.cat(outs)

        dt, got = timed(stream)
        assert torch.equal(got, want), f"block {block}: the stream is not the one-shot decode"
        steady = per_push[(hr + block - 1) // block + 1:] or per_push
        res[f"stream_block_{block}"] = {"ms": 1e3 * dt, "rtf": dt / audio_s, "vs_one_shot": dt / (res["one_shot"]["ms"] / 1e3), "pushes": len(per_push),
                                        "push_ms_mean": 1e3 * sum(steady) / len(steady), "push_ms_max": 1e3 * max(steady),
                                        "block_ms_of_audio": 1e3 * block * m.hop_length / m.sample_rate,
                                        "frames_decoded_per_frame": stream.st.frames_decoded / T, "predicted_recompute_share": (block + hl + hr) / block,
                                        "delay_ms": 1e3 * stream.st.delay_samples / m.sample_rate}
    dt, got = timed(lambda: m.decode_long(codes, window_frames=a.window_frames, rows_per_call=a.rows_per_call)[0, 0])
    assert torch.equal(got, want), "decode_long is not the one-shot decode"
    blk = a.window_frames - hl - hr
    res["decode_long"] = {"ms": 1e3 * dt, "rtf": dt / audio_s, "vs_one_shot": dt / (res["one_shot"]["ms"] / 1e3), "window_frames": a.window_frames,
                          "rows_per_call": a.rows_per_call, "predicted_recompute_share": a.window_frames / blk,
                          "workspace_mib": ws_bytes(a.rows_per_call, a.window_frames) / 2 ** 20, "one_shot_workspace_mib": ws_bytes(1, T) / 2 ** 20}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
