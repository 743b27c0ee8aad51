"""The segmental SNRs on the GPU (csrc/segsnr.hip) against the float64 yardstick of flowdec_amd.segsnr, over the case set of
tests/test_segsnr_cpu.py (CASES): three rates (N 512 with two frames per workgroup, N 1024, N 4096), frame counts 1, 6, 7, 62 and 289, a
clip under win + skip, noise from 40 to -15 dB, a silent stretch in x, and the two contents a packed float32 transform gets wrong without
the per-frame scaling: a zeroed tail and a head at 1e-6 in x_hat only.

SSNR, per frame and per clip: within SS_TOL = 1e-9 dB.  Derived, not measured: both sides form w x, w x_hat and their difference with the
same roundings and add at most 1440 non-negative float64 terms, relative 1440 * 2^-53 = 1.6e-13 on each energy whatever the order, which
is 10 log10(e) * 3.2e-13 = 1.4e-12 dB behind the logarithm (whose argument's + eps terms and the clip are continuous); 1e-9 leaves room
for the two libraries' log10.

fwSSNR rests on the float32 transform.  Measured on an MI355X over the case set (MEASUREMENTS.md "Segmental SNRs"): the worst clip deviates
FW_CLIP_MEASURED = 2.575e-05 dB (8 kHz, zeroed tail), the worst frame FW_FRAME_MEASURED = 1.528e-03 dB (16 kHz, zeroed tail; a frame that
straddles the edge of the silence); the tolerances are 8 times those (seeds and lengths not in the set), and the
clip tolerance may not exceed 1e-3 dB, the digits of the CSV.  On a build without the scaling test_against_the_yardstick fails: the 'tail'
clips are off by 0.13 and 0.21 dB, the 'head' clips by 0.15 dB, single frames by up to 3.7 dB (measured once with such a library)."""
import ctypes as C

import numpy as np
import pytest
import torch

from test_eval_cpu import read_csv, write_wav
from test_segsnr_cpu import CASES, DIMS, RATES, case_pairs, pair

pytestmark = pytest.mark.gpu

FD_EINVAL = -1
SS_TOL = 1e-9
FW_CLIP_MEASURED, FW_FRAME_MEASURED = 2.575e-05, 1.528e-03
FW_CLIP_TOL, FW_FRAME_TOL = 8 * FW_CLIP_MEASURED, 8 * FW_FRAME_MEASURED
assert FW_CLIP_TOL <= 1e-3


@pytest.fixture(scope="module")
def clips():
    """Per rate: the seeded pairs, their cases and their float64 detail, computed once and never changed."""
    from flowdec_amd import segsnr
    out = {}
    for sr in RATES:
        pairs, cases = case_pairs(sr)
        out[sr] = (pairs, cases, [segsnr.segsnr_detail(h, x, sr) for h, x in pairs])
    return out


def plan_of(sr):
    from flowdec_amd import segsnr
    return segsnr.segsnr_plan(sr, "cuda")


def stage(pairs, Lrow=None):
    from flowdec_amd.batching import padded_rows
    Lrow = Lrow or max(len(x) for _, x in pairs)
    rh, lens = padded_rows([torch.from_numpy(h) for h, _ in pairs], Lrow, "cuda")
    rx, _ = padded_rows([torch.from_numpy(x) for _, x in pairs], Lrow, "cuda")
    return rh, rx, lens, Lrow


def run(sr, pairs, lens_override=None, Lrow=None):
    """fd_metrics_segsnr on one batch -> (out [B, 2], frames [B, T, 2]) as host arrays."""
    from flowdec_amd import _lib as L
    lib, plan = L.load(), plan_of(sr)
    rh, rx, lens, Lrow = stage(pairs, Lrow)
    if lens_override is not None:
        lens = torch.tensor(lens_override, dtype=torch.int32, device="cuda")
    B, T = len(pairs), max((Lrow - plan.win) // plan.skip, 0)
    nws = lib.fd_metrics_segsnr_workspace_bytes(plan.handle, B, Lrow)
    assert nws > 0
    ws = torch.empty(nws, dtype=torch.uint8, device="cuda")
    out = torch.full((B, 2), -7.0, dtype=torch.float64, device="cuda")
    frames = torch.full((B, max(T, 1), 2), -7.0, dtype=torch.float64, device="cuda")
    L.check(lib.fd_metrics_segsnr(plan.handle, L.ptr(rh), L.ptr(rx), L.ptr(lens), B, Lrow, L.ptr(out), L.ptr(frames), L.ptr(ws), nws, L.stream()))
    torch.cuda.synchronize()
    return out.cpu().numpy(), frames.cpu().numpy()[:, :T]


def test_against_the_yardstick(clips):
    worst = dict(fw_clip=0.0, fw_frame=0.0, ss_clip=0.0, ss_frame=0.0)
    seen_T = set()
    for sr in RATES:
        pairs, cases, dets = clips[sr]
        out, frames = run(sr, pairs)
        for b, ((_, n, kind), d) in enumerate(zip(cases, dets)):
            T = d["frames"]
            seen_T.add((sr, T))
            assert T == max((n - DIMS[sr][0]) // DIMS[sr][1], 0) and np.all(np.isnan(frames[b, T:]))      # frames the clip does not have
            if T == 0:
                assert np.all(np.isnan(out[b]))
                continue
            e = dict(fw_clip=abs(out[b, 0] - d["fwssnr"]), ss_clip=abs(out[b, 1] - d["ssnr"]),
                     fw_frame=float(np.abs(frames[b, :T, 0] - d["fw_frames"]).max()), ss_frame=float(np.abs(frames[b, :T, 1] - d["ss_frames"]).max()))
            print(f"segsnr {sr} Hz {n} samples ({kind}), T {T}: fwSSNR {out[b, 0]:.9f} err {e['fw_clip']:.2e} (worst frame {e['fw_frame']:.2e}); "
                  f"SSNR {out[b, 1]:.9f} err {e['ss_clip']:.2e} (worst frame {e['ss_frame']:.2e})")
            for k in worst:
                worst[k] = max(worst[k], e[k])
            assert -10 <= frames[b, :T].min() and frames[b, :T].max() <= 35
    print(f"segsnr worst over the case set: fwSSNR clip {worst['fw_clip']:.3e} dB, frame {worst['fw_frame']:.3e} dB; "
          f"SSNR clip {worst['ss_clip']:.3e} dB, frame {worst['ss_frame']:.3e} dB")
    assert {(8000, 0), (8000, 1), (8000, 6), (8000, 7), (8000, 62), (8000, 289), (16000, 1), (16000, 62), (48000, 29)} <= seen_T
    assert worst["ss_clip"] <= SS_TOL and worst["ss_frame"] <= SS_TOL
    assert worst["fw_clip"] <= FW_CLIP_TOL and worst["fw_frame"] <= FW_FRAME_TOL


def test_batch_invariance_bit_for_bit(clips):
    from flowdec_amd import segsnr
    for sr in (8000, 16000):
        pairs, cases, _ = clips[sr]
        full, fr_full = run(sr, pairs)
        rev, fr_rev = run(sr, pairs[::-1])
        assert np.array_equal(rev[::-1], full, equal_nan=True)                                                # at another row
        longest = max(range(len(pairs)), key=lambda i: len(pairs[i][1]))
        for b, p in enumerate(pairs):
            T = max((len(p[1]) - DIMS[sr][0]) // DIMS[sr][1], 0)
            o1, f1 = run(sr, [p])                                                                             # alone
            o2, f2 = run(sr, [pairs[longest], p, pairs[0]])                                                   # beside clips of other lengths
            assert np.array_equal(o1[0], full[b], equal_nan=True) and np.array_equal(o2[1], full[b], equal_nan=True)
            assert np.array_equal(f1[0, :T], fr_full[b, :T]) and np.array_equal(f2[1, :T], fr_full[b, :T]) and np.array_equal(fr_rev[len(pairs) - 1 - b, :T], fr_full[b, :T])
        hs, xs = [h for h, _ in pairs], [x for _, x in pairs]
        a = segsnr.segsnr_batch(hs, xs, sr, batch=3)
        c, fc = segsnr.segsnr_batch(hs, xs, sr, batch=8, return_frames=True)
        assert a.shape == (len(pairs), 2) and np.array_equal(a, c, equal_nan=True) and np.array_equal(c, full, equal_nan=True)
        for b, p in enumerate(pairs):
            T = max((len(p[1]) - DIMS[sr][0]) // DIMS[sr][1], 0)
            assert fc[b].shape == (T, 2) and np.array_equal(fc[b], fr_full[b, :T])


def test_identity_and_scaling(clips):
    """x_hat = x scores exactly 35.0 in both columns on a clip without silence.  Scaling both signals by 2^k changes no bit of fwSSNR on the
    noise clips (every sample far above eps, so x + eps scales with x to the last bit of the float32 rounding)."""
    for sr in RATES:
        pairs, cases, _ = clips[sr]
        keep = [i for i, (_, n, kind) in enumerate(cases) if not isinstance(kind, str) and n >= sum(DIMS[sr][:2])] or [0]
        noisy = [pairs[i] for i in keep] if sr != 48000 else [pair(3000, sr, 77, 10)]
        out, frames = run(sr, [(x, x) for _, x in noisy])
        assert np.all(out == 35.0) and np.all(frames[~np.isnan(frames)] == 35.0)
        base, fr_base = run(sr, noisy)
        for k in (3, -7):
            got, fr = run(sr, [((h * 2.0 ** k).astype(np.float32), (x * 2.0 ** k).astype(np.float32)) for h, x in noisy])
            assert np.array_equal(got[:, 0], base[:, 0]) and np.array_equal(fr[..., 0], fr_base[..., 0], equal_nan=True)
            assert np.all(np.abs(got[:, 1] - base[:, 1]) < 1e-6)                                              # SSNR: eps beside the noise energy


def test_refusals_leave_the_outputs_untouched(clips):
    from flowdec_amd import _lib as L
    lib = L.load()
    sr = 8000
    pairs, cases, _ = clips[sr]
    plan = plan_of(sr)
    err = lambda: lib.fd_last_error().decode()
    rh, rx, lens, Lrow = stage(pairs)
    B, T = len(pairs), (Lrow - 240) // 60
    nws = lib.fd_metrics_segsnr_workspace_bytes(plan.handle, B, Lrow)
    assert lib.fd_metrics_segsnr_workspace_bytes(plan.handle, 0, Lrow) == 0 and lib.fd_metrics_segsnr_workspace_bytes(plan.handle, 65536, Lrow) == 0
    assert lib.fd_metrics_segsnr_workspace_bytes(plan.handle, B, 0) == 0 and lib.fd_metrics_segsnr_workspace_bytes(plan.handle, B, 100) > 0
    ws = torch.empty(nws, dtype=torch.uint8, device="cuda")
    out = torch.full((B, 2), -7.0, dtype=torch.float64, device="cuda")
    frames = torch.full((B, T, 2), -7.0, dtype=torch.float64, device="cuda")
    p = L.ptr
    call = lambda plan_=plan.handle, xh=p(rh), x=p(rx), ln=p(lens), B_=B, L_=Lrow, o=p(out), w=p(ws), n=nws: \
        lib.fd_metrics_segsnr(plan_, xh, x, ln, B_, L_, o, p(frames), w, n, L.stream())
    assert call(plan_=None) == FD_EINVAL and "null pointer" in err()
    assert call(xh=None) == FD_EINVAL and "null pointer" in err()
    assert call(x=None) == FD_EINVAL and call(ln=None) == FD_EINVAL and call(o=None) == FD_EINVAL and call(w=None) == FD_EINVAL and "null pointer" in err()
    assert call(B_=0) == FD_EINVAL and "bad batch B 0" in err()
    assert call(L_=0) == FD_EINVAL and "bad batch" in err()
    assert call(n=nws - 1) == FD_EINVAL and "workspace too small" in err()
    h = C.c_void_p()
    assert lib.fd_segsnr_plan_create(96000, C.byref(h)) == FD_EINVAL and "outside [128, 4096]" in err() and not h.value
    torch.cuda.synchronize()
    assert torch.all(out == -7.0) and torch.all(frames == -7.0)
    # a device length the host cannot see: under win + skip, beyond the row, 0 and negative give NaN for that clip alone
    good, good_fr = run(sr, pairs)
    short = [i for i, (_, n, _) in enumerate(cases) if n < 300]
    assert short == [3] and np.all(np.isnan(good[3])) and np.all(np.isfinite(np.delete(good, 3, axis=0)))
    for bad in (299, Lrow + 1, 0, -5):
        ln = [n for _, n, _ in cases]
        ln[1] = bad
        o, f = run(sr, pairs, lens_override=ln)
        assert np.all(np.isnan(o[1])) and np.all(np.isnan(f[1]))
        keep = [i for i in range(B) if i != 1]
        assert np.array_equal(o[keep], good[keep], equal_nan=True) and np.array_equal(f[keep], good_fr[keep], equal_nan=True)
    # rows shorter than win + skip: no frame kernel at all, NaN everywhere
    o, f = run(sr, [pairs[3]])
    assert np.all(np.isnan(o)) and f.shape == (1, 0, 2)


def test_eval_cli_ssnr_end_to_end(tmp_path, capsys):
    from flowdec_amd import eval_cli
    sr = 8000
    lines = []
    for i, (n, kind) in enumerate(((2000, 15), (4000, "tail"), (280, 20), (3001, 5))):            # 0.25 s, 0.5 s, one under 300 samples, 0.375 s
        h, x = pair(n, sr, 60 + i, kind)
        y = (x + 0.1 * np.random.default_rng(100 + i).standard_normal(n)).astype(np.float32)
        paths = [tmp_path / f"clean_{i}.wav", tmp_path / f"noisy_{i}.wav", tmp_path / f"enh_{i}.wav"]
        for path, s in zip(paths, (x, y, h)):
            write_wav(path, s, sr)
        lines.append(" ---> ".join(str(q) for q in paths))
    lst = tmp_path / "triples_list.txt"
    lst.write_text("\n".join(lines) + "\n")
    gpu, host = tmp_path / "gpu.csv", tmp_path / "host.csv"
    argv = ["--triples", str(lst), "--batch-files", "3", "--sr", str(sr), "--ssnr"]
    r_gpu = eval_cli.run(argv + ["--out", str(gpu)])
    cap = capsys.readouterr()
    eval_cli.run(argv + ["--out", str(host)], scorer=eval_cli.HOST_SCORER)
    (hg, rg), (hh, rh) = read_csv(gpu), read_csv(host)
    assert hg == hh == list(eval_cli.CSV_HEADER) + ["fwSSNR", "SSNR"] and len(rg) == 4
    assert cap.out.count("mean =") == 6 and "fwSSNR" in cap.out and "300 samples" in cap.err and "enh_2.wav" in cap.err
    assert rg[2][-2:] == ["nan", "nan"] and rh[2][-2:] == ["nan", "nan"] and r_gpu.means[-1][2] == 3 and r_gpu.means[-2][2] == 3
    for i in (0, 1, 3):
        assert abs(float(rg[i][-2]) - float(rh[i][-2])) <= FW_CLIP_TOL and abs(float(rg[i][-1]) - float(rh[i][-1])) <= SS_TOL
        assert -10 < float(rg[i][-2]) < 35 and -10 < float(rg[i][-1]) < 35
