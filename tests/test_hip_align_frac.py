"""Sub-sample alignment on the GPU (csrc/xcorr.hip fd_xcorr_lags_frac, csrc/fracshift.hip fd_frac_shift) against the float64 yardsticks of
flowdec_amd.align.  Every comparison is exact: the refinement and the shift are defined with their order of operations (taps ascending,
products and sums separately rounded float64), so the device must give the yardstick's bits.

* lag_q and sign equal refine_lag of the DEVICE's own c (the correlation itself is only bounded against the host's, tests/test_hip_align.py),
  and that c equals fd_xcorr_lags' c bit for bit.
* fd_frac_shift equals frac_shift bit for bit.

Shapes: lengths 1, 2 W - 1, 2 W, 257 and one correlation slice -+ 1 (32767, 32769: also 33 output tiles of the shift, the last one
partial); M = 8 (the taps run off both ends of c) and M = 40 (inside); a peak at |l0| = M; silent signals; j = 1 and j = Q - 1; negative
base; windows that start before the signal, end behind it and lie wholly outside it."""
import io

import numpy as np
import pytest
import torch

from test_align_cpu import FD_EINVAL, FD_ENOMEM, SR, shifted
from test_align_frac_cpu import delayed_pair, frac_triples
from test_eval_cpu import read_csv, write_wav
from test_hip_align import gpu_xcorr, rows_of

pytestmark = pytest.mark.gpu

Q, W = 64, 32
LENGTHS = (1, 2 * W - 1, 2 * W, 257, 32767, 32769)
DELAYS = (0.5, -3.625, 2.3, -5.25)        # of the band-limited pairs, by i % 4


def gpu_frac(pairs, M, polarity, q=Q, w=W, La=None, Lb=None, want_c=True):
    """fd_xcorr_lags_frac on one batch -> (c float64 [B, 2 M + 1] or None, lag_q int64 [B], sign int32 [B]) as host arrays."""
    from flowdec_amd import _lib as L, align
    lib = L.load()
    B = len(pairs)
    La, Lb = La or max(len(a) for a, _ in pairs), Lb or max(len(b) for _, b in pairs)
    ra, rb = rows_of([a for a, _ in pairs], La), rows_of([b for _, b in pairs], Lb)
    la, lb = (torch.tensor(v, dtype=torch.int32, device="cuda") for v in ([len(a) for a, _ in pairs], [len(b) for _, b in pairs]))
    bank = torch.tensor(align.frac_bank(q, w)).cuda()
    nws = lib.fd_xcorr_frac_workspace_bytes(B, La, Lb, M)
    assert nws > 0
    ws = torch.empty(nws, dtype=torch.uint8, device="cuda")
    c = torch.full((B, 2 * M + 1), -7.0, dtype=torch.float64, device="cuda") if want_c else None
    lag_q = torch.full((B,), -77, dtype=torch.int64, device="cuda")
    sign = torch.full((B,), -77, dtype=torch.int32, device="cuda")
    L.check(lib.fd_xcorr_lags_frac(L.ptr(ra), L.ptr(rb), L.ptr(la), L.ptr(lb), B, La, Lb, M, L.ptr(bank), q, w, int(polarity), L.ptr(c), L.ptr(lag_q),
                                   L.ptr(sign), L.ptr(ws), nws, L.stream()))
    torch.cuda.synchronize()
    return (c.cpu().numpy() if want_c else None), lag_q.cpu().numpy(), sign.cpu().numpy()


def gpu_shift(signals, lag_q, sign, windows, q=Q, w=W, Ls=None, Lo=None):
    """fd_frac_shift on one batch -> float32 [B, Lo] as a host array (the whole rows: the tail behind each window included)."""
    from flowdec_amd import _lib as L, align
    lib = L.load()
    B = len(signals)
    Ls, Lo = Ls or max(max(len(s) for s in signals), 1), Lo or max(max(b - a for a, b in windows), 1)
    H = align.frac_bank(q, w)
    rows = rows_of(signals, Ls, fill=float("nan"))                 # a poisoned tail: samples behind a clip are zeros by definition, never loaded
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device="cuda")
    lens, base, sg, n0, n1 = i32([len(s) for s in signals]), i32([l // q for l in lag_q]), i32(list(sign)), i32([a for a, _ in windows]), i32([b for _, b in windows])
    taps = torch.from_numpy(np.stack([H[l % q] for l in lag_q])).cuda()
    out = torch.full((B, Lo), 7.0, dtype=torch.float32, device="cuda")
    L.check(lib.fd_frac_shift(L.ptr(rows), L.ptr(lens), B, Ls, L.ptr(base), L.ptr(taps), w, L.ptr(sg), L.ptr(n0), L.ptr(n1), L.ptr(out), Lo, L.stream()))
    torch.cuda.synchronize()
    return out.cpu().numpy()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.int32 if a.dtype == np.float32 else np.int64),
                                                                       b.view(np.int32 if b.dtype == np.float32 else np.int64))


def noise_pair(L, d, seed, invert=False):
    """Lengths too short for delayed_pair's band limiting: white noise and its whole-sample shift plus a little noise."""
    rng = np.random.default_rng(seed)
    a = rng.standard_normal(L).astype(np.float32)
    b = (-1.0 if invert else 1.0) * shifted(a, d) + (0.05 * rng.standard_normal(L)).astype(np.float32)
    return a, b.astype(np.float32)


@pytest.fixture(scope="module")
def pairs():
    """One pair per length of LENGTHS: sub-sample delays where the length allows band-limited noise, every second one inverted."""
    out = []
    for i, L in enumerate(LENGTHS):
        out.append(delayed_pair(L, DELAYS[i % 4], 0.9, 300 + i, invert=bool(i % 2)) if L >= 257 else noise_pair(L, i % 2, 300 + i, invert=bool(i % 2)))
    return out


@pytest.mark.parametrize("M", [8, 40])
@pytest.mark.parametrize("polarity", [False, True])
def test_lag_q_and_sign_equal_refine_lag_of_the_device_c(pairs, M, polarity):
    from flowdec_amd import align
    c, lag_q, sign = gpu_frac(pairs, M, polarity)
    c_int, lags_int = gpu_xcorr(pairs, M)
    assert same_bits(c, c_int)                                                  # the correlation of fd_xcorr_lags, bit for bit
    for i, (a, b) in enumerate(pairs):
        want = align.refine_lag(c[i], Q, W, polarity)
        assert (int(lag_q[i]), int(sign[i])) == want, (len(a), M, polarity, want)
        if not polarity:
            assert abs(int(lag_q[i]) - int(lags_int[i]) * Q) < Q and sign[i] == 1
    if polarity and M == 40:                                                    # every tap inside c: the long clips' delays to the grid step
        for i in (4, 5):
            assert abs(lag_q[i] / Q - DELAYS[i % 4]) <= 1.0 / Q and sign[i] == (-1 if i % 2 else 1), (i, lag_q[i] / Q)
    # c = NULL: the same lags
    _, lq2, sg2 = gpu_frac(pairs, M, polarity, want_c=False)
    assert np.array_equal(lq2, lag_q) and np.array_equal(sg2, sign)


def test_peak_at_the_edge_silence_and_other_grids():
    from flowdec_amd import align
    rng = np.random.default_rng(7)
    a = rng.standard_normal(700).astype(np.float32)
    silent = np.zeros(500, np.float32)
    for M in (8, 40):
        cases = [(a, shifted(a, M)), (a, -shifted(a, -M)), (silent, silent[:300]), (a, shifted(a, M + 5))]
        c, lag_q, sign = gpu_frac(cases, M, True)
        for i in range(4):
            assert (int(lag_q[i]), int(sign[i])) == align.refine_lag(c[i], Q, W, True), (M, i)
        assert abs(lag_q[0]) <= M * Q and lag_q[0] > (M - 1) * Q and -M * Q <= lag_q[1] < -(M - 1) * Q and sign[:3].tolist() == [1, -1, 1]
        assert lag_q[2] == 0 and np.all(c[2] == 0.0)
    # the smallest and the largest grid the entry point takes, and an odd one
    x, y = delayed_pair(2000, 1.37, 0.8, 11, True)
    for q, w in ((2, 1), (1024, 256), (10, 5)):
        c, lag_q, sign = gpu_frac([(x, y)], 300, True, q=q, w=w)
        assert (int(lag_q[0]), int(sign[0])) == align.refine_lag(c[0], q, w, True) and sign[0] == -1
        assert 0 < lag_q[0] < 2 * q                                             # the integer peak is 1: the refined lag lies within a sample of it


@pytest.mark.parametrize("k", range(len(LENGTHS)))
def test_frac_shift_equals_the_yardstick_bit_for_bit(pairs, k):
    from flowdec_amd import align
    s = pairs[k][1]
    L = len(s)
    # (lag_q, sign, n0, n1): j = 1, j = Q - 1 with a negative base, a whole delay with sign -1, the support itself, windows over both ends
    cases = [(1, 1, 0, L), (-3 * Q - 1, -1, 0, L), (5 * Q, -1, -7, L + 9), (2 * Q + 33, 1, -40, L - 1), (-Q + 17, -1, 3, L + 70)]
    lo, hi = align.support_frac(L, 2 * Q + 33, Q, W)
    if hi > lo:
        cases.append((2 * Q + 33, 1, lo, hi))
    got = gpu_shift([s] * len(cases), [c[0] for c in cases], [c[1] for c in cases], [(c[2], c[3]) for c in cases])
    for i, (lag_q, sign, n0, n1) in enumerate(cases):
        want = align.frac_shift(s, lag_q, sign, Q, W, n0, n1)
        assert same_bits(got[i, :n1 - n0], want), (L, cases[i])
        assert not got[i, n1 - n0:].any()                                       # zeros behind the window
    if L > 5:
        assert np.array_equal(got[2, 7:7 + L - 5], -s[5:])                      # j = 0 and sign -1: the negated samples themselves


def test_windows_outside_the_signal_and_clamped_tables():
    from flowdec_amd import align
    rng = np.random.default_rng(3)
    s = rng.standard_normal(300).astype(np.float32)
    # wholly behind, wholly before, empty, reversed; a window longer than the output row is cut to the row
    cases = [(Q + 5, 1, 500, 700), (Q + 5, -1, -900, -700), (Q + 5, 1, 10, 10), (Q + 5, 1, 50, 20), (Q + 5, 1, 0, 5000)]
    got = gpu_shift([s] * 5, [c[0] for c in cases], [c[1] for c in cases], [(c[2], c[3]) for c in cases], Lo=256)
    assert not got[:4].any() and same_bits(got[4], align.frac_shift(s, Q + 5, 1, Q, W, 0, 256))
    # lengths beyond the row and below zero are clamped; a base of +-2^31 reads only zeros: the call returns normally
    from flowdec_amd import _lib as L
    lib = L.load()
    rows = rows_of([s, s, s], 300)
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device="cuda")
    taps = torch.from_numpy(np.stack([align.frac_bank(Q, W)[9]] * 3)).cuda()
    out = torch.full((3, 200), 7.0, device="cuda")
    lens, base, sg, n0, n1 = i32([0x7fffffff, -4, 300]), i32([0, 0, -0x80000000]), i32([1, 1, 1]), i32([0, 0, 0x7fffffff]), i32([200, 200, -0x80000000])
    L.check(lib.fd_frac_shift(L.ptr(rows), L.ptr(lens), 3, 300, L.ptr(base), L.ptr(taps), W, L.ptr(sg), L.ptr(n0), L.ptr(n1), L.ptr(out), 200, L.stream()))
    torch.cuda.synchronize()
    out = out.cpu().numpy()
    assert same_bits(out[0], align.frac_shift(s, 9, 1, Q, W, 0, 200)) and not out[1:].any()


def test_batch_independence_bit_for_bit(pairs):
    clip = pairs[3]                                                              # 257 samples
    others = [pairs[4], pairs[1], pairs[5]]
    M = 40
    alone = gpu_frac([clip], M, True)
    first = gpu_frac([clip] + others, M, True)
    fourth = gpu_frac(others + [clip], M, True, La=40000, Lb=33333)               # longer rows too: a slice more that no clip has
    for got, j in ((first, 0), (fourth, 3)):
        assert same_bits(got[0][j], alone[0][0]) and got[1][j] == alone[1][0] and got[2][j] == alone[2][0]
    s, args = clip[1], (Q + 1, -1, (-5, 300))
    sig = [o[1] for o in others]
    one = gpu_shift([s], [args[0]], [args[1]], [args[2]])
    lead = gpu_shift([s] + sig, [args[0], 7, -200, 3 * Q], [args[1], 1, 1, -1], [args[2], (0, 32767), (10, 50), (0, 33000)])
    last = gpu_shift(sig + [s], [7, -200, 3 * Q, args[0]], [1, 1, -1, args[1]], [(0, 32767), (10, 50), (0, 33000), args[2]], Ls=40000)
    assert same_bits(lead[0, :305], one[0]) and same_bits(last[3, :305], one[0]) and not lead[0, 305:].any() and not last[3, 305:].any()


def test_refusals_launch_nothing(pairs):
    from flowdec_amd import _lib as L, align
    lib = L.load()
    a, b = pairs[3]
    ra, rb = rows_of([a], 257), rows_of([b], 257)
    la = torch.tensor([257], dtype=torch.int32, device="cuda")
    bank = torch.tensor(align.frac_bank(Q, W)).cuda()
    nws = lib.fd_xcorr_frac_workspace_bytes(1, 257, 257, 40)
    ws = torch.zeros(nws, dtype=torch.uint8, device="cuda")
    c = torch.full((1, 81), -7.0, dtype=torch.float64, device="cuda")
    lag_q = torch.full((1,), -77, dtype=torch.int64, device="cuda")
    sign = torch.full((1,), -77, dtype=torch.int32, device="cuda")
    call = lambda bank=L.ptr(bank), q=Q, w=W, n=nws: lib.fd_xcorr_lags_frac(L.ptr(ra), L.ptr(rb), L.ptr(la), L.ptr(la), 1, 257, 257, 40, bank, q, w, 1, L.ptr(c),
                                                                             L.ptr(lag_q), L.ptr(sign), L.ptr(ws), n, L.stream())
    err = lambda: lib.fd_last_error().decode()
    assert call(bank=None) == FD_EINVAL and "bank" in err()
    assert call(q=1) == FD_EINVAL and "Q 1" in err() and call(w=0) == FD_EINVAL and "W 0" in err()
    assert call(n=nws - 1) == FD_ENOMEM and "workspace" in err()
    out = torch.full((1, 300), 7.0, device="cuda")
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device="cuda")
    z = i32([0])
    assert lib.fd_frac_shift(L.ptr(rb), L.ptr(la), 1, 257, L.ptr(z), L.ptr(bank), 0, L.ptr(z), L.ptr(z), L.ptr(la), L.ptr(out), 300, L.stream()) == FD_EINVAL
    assert lib.fd_frac_shift(L.ptr(rb), L.ptr(la), 1, 257, L.ptr(z), None, W, L.ptr(z), L.ptr(z), L.ptr(la), L.ptr(out), 300, L.stream()) == FD_EINVAL
    torch.cuda.synchronize()
    assert (c == -7.0).all() and lag_q.item() == -77 and sign.item() == -77 and not ws.any() and (out == 7.0).all()
    assert call() == 0
    torch.cuda.synchronize()
    assert lag_q.item() != -77 and sign.item() == -1


def test_wrappers_agree_with_the_entry_points_and_the_host(pairs):
    from flowdec_amd import align
    M = 40
    as_, bs = [torch.from_numpy(a) for a, _ in pairs], [torch.from_numpy(b) for _, b in pairs]
    c, lag_q, sign = gpu_frac(pairs, M, True)
    wq, wsg, wc = align.lags_batch_frac(as_, bs, M, Q, W, True, batch=4, return_xcorr=True)
    assert wq.dtype == np.int64 and wsg.dtype == np.int32 and np.array_equal(wq, lag_q) and np.array_equal(wsg, sign) and same_bits(wc, c)
    wq2, wsg2 = align.lags_batch_frac(as_, bs, M, Q, W, True, batch=1)
    assert np.array_equal(wq2, wq) and np.array_equal(wsg2, wsg)
    windows = [(-3, len(b) + 5) for _, b in pairs]
    lq = [int(l) + 1 for l in lag_q]
    got = align.shift_batch(bs, lq, sign, windows, Q, W, batch=4)
    want = align.host_shift(bs, lq, sign, windows, Q, W)
    assert all(g.dtype == torch.float32 and same_bits(g.numpy(), h.numpy()) for g, h in zip(got, want))
    with pytest.raises(ValueError):
        align.lags_batch_frac(as_, bs, M, 1, W)
    with pytest.raises(ValueError):
        align.shift_batch(bs, lq[:-1], sign, windows, Q, W)


def test_eval_cli_align_frac_end_to_end(tmp_path, capsys):
    from flowdec_amd import eval_cli
    lst = frac_triples(tmp_path)
    flags = ["--batch-files", "2", "--align", "1", "--align-frac", "--align-polarity"]
    r = eval_cli.run(["--triples", str(lst), "--out", str(tmp_path / "gpu.csv")] + flags)
    eval_cli.run(["--triples", str(lst), "--out", str(tmp_path / "host.csv")] + flags, scorer=eval_cli.HOST_SCORER)
    eval_cli.run(["--triples", str(lst), "--out", str(tmp_path / "int.csv"), "--batch-files", "2", "--align", "1"])
    capsys.readouterr()
    (hg, rg), (hh, rh), (hi, ri) = read_csv(tmp_path / "gpu.csv"), read_csv(tmp_path / "host.csv"), read_csv(tmp_path / "int.csv")
    assert hg == hh == list(eval_cli.CSV_HEADER) + ["lag_x_hat", "lag_y", "pol_x_hat", "pol_y"]
    assert [row[-4:] for row in rg] == [row[-4:] for row in rh] == [["2.5", "-3", "-1", "1"], ["4", "-2", "1", "1"]]
    assert r.lags == [("lag_x_hat", "2.5", "4", 2), ("lag_y", "-3", "-2", 2)] and r.inverted == [("pol_x_hat", 1), ("pol_y", 0)]
    assert float(rg[0][4]) > 30.0 > float(ri[0][4])
    assert rg[1][:-2] == ri[1]                                                   # whole delays: the bits of --align


def test_estimate_cli_and_loss_cli_align_their_pairs(tmp_path, capsys):
    """Two pairs at 48 kHz, the second delayed by 2.5 samples and inverted: both programs run, stdout keeps its shape, and the summary line
    on stderr reports the lag and the inversion."""
    from flowdec_amd import estimate_cli, loss_cli
    from test_cli import synthetic_ckpt
    lines = []
    for i, (d, inv) in enumerate(((0.0, False), (2.5, True))):
        x, y = delayed_pair(12500, d, 0.8, 50 + i, inv)
        write_wav(tmp_path / f"x{i}.wav", 0.3 * x, SR)
        write_wav(tmp_path / f"y{i}.wav", 0.3 * y, SR)
        lines.append(f"{tmp_path / f'x{i}.wav'} ---> {tmp_path / f'y{i}.wav'}")
    pairs = tmp_path / "pairs.txt"
    pairs.write_text("\n".join(lines) + "\n")
    want = "align: lag min = 0  max = 2.5 samples (coded against clean, positive = late), non-zero in 1 of 2 pairs, 1 inverted"
    buf = io.StringIO()
    common = ["--pairs-file", str(pairs), "--alpha", "0.3", "--nfft", "1534", "--hop", "384", "--n-samples", "2", "--sample-duration", "0.25", "--per-band"]
    res = estimate_cli.run(common + ["--align", "1", "--align-frac", "--align-polarity", "--outfile-suffix", "frac"], out=buf)
    assert res is not None and want in capsys.readouterr().err and buf.getvalue().splitlines()[2] == "=== Results ===" and "align" not in buf.getvalue().split("Args:")[0]
    plain = estimate_cli.run(common, out=io.StringIO())
    assert "align:" not in capsys.readouterr().err
    top = slice(600, 700)                                                       # unaligned: the upper bands hold the delay and the inversion
    assert np.isfinite(res.sigma_y).all() and float(np.mean(res.sigma_y[top])) < 0.1 * float(np.mean(plain.sigma_y[top]))
    torch.save(synthetic_ckpt(), tmp_path / "m.ckpt")
    base = ["--ckpt", str(tmp_path / "m.ckpt"), "--pairs-file", str(pairs), "--no-crop", "--seed", "9", "--batch", "2"]
    buf = io.StringIO()
    got = loss_cli.run(base + ["--align", "1", "--align-frac", "--align-polarity"], out=buf)
    assert want in capsys.readouterr().err and buf.getvalue().startswith("valid_loss = ") and len(buf.getvalue().splitlines()) == 1
    assert np.isfinite(got.per_pair).all() and len(got.per_pair) == 2
    raw = loss_cli.run(base, out=io.StringIO())
    assert "align:" not in capsys.readouterr().err and got.per_pair[0] == raw.per_pair[0] and got.per_pair[1] != raw.per_pair[1]
