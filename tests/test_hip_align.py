"""The bounded-lag cross-correlation on the GPU (csrc/xcorr.hip) against the float64 yardstick of flowdec_amd.align.

Exact-integer data: a = integers in [-64, 64], b = a shifted by d (zero where nothing lands) plus integers in [-8, 8].  Every sum is an
integer far below 2^53, so the GPU's c must equal the yardstick BIT FOR BIT in any order of addition, and the lag must be d (the peak is
more than 10 times the runner-up in each case).
Float data: per lag |c_gpu - c_ref| <= n_l 2^-52 sum_n |a[n] b[n + l]| with n_l the number of terms of that lag -- the textbook bound for
any order of summation of exactly representable products (each side at most (n_l - 1) 2^-53 of that sum), derived and not measured.

The shapes are the smallest at which the kernel can still go wrong: lengths that are no multiple of any tile, unequal La / Lb in both
directions, peaks at both edges of the search; the last two exact cases are this kernel's own (more than one 2048-lag tile, more than one
32768-sample slice, chunks that the tile's lags cannot meet; a clip that ends exactly on a slice boundary)."""
import ctypes as C

import numpy as np
import pytest
import torch

from test_align_cpu import ADVANCE_Y, DELAY_H, SR, make_delayed_triples, shifted
from test_eval_cpu import read_csv, write_wav

pytestmark = pytest.mark.gpu

CASES = [(4097, 4100, 300, 300), (9001, 8990, 300, -300), (1000, 1000, 17, 0), (700, 1300, 600, 257), (5000, 5000, 1, -1)]     # (La, Lb, M, d)
# 3 slices of a, 3 lag tiles, the clip of b ends inside the second slice's reach; a clip that ends exactly on a slice boundary (the lag
# offsets 1 .. 15 of a 16-lag group then need one slice more)
OWN_CASES = [(70001, 66000, 2500, -2311), (32768, 33000, 40, 33)]
SEEDS = (100, 110, 121, 1010, 140, 150, 160)    # chosen on the host so that every peak is more than 10 times the runner-up (asserted below)


def integer_pair(La, Lb, d, seed):
    rng = np.random.default_rng(seed)
    a = rng.integers(-64, 65, La).astype(np.float32)
    return a, shifted(a, d, length=Lb) + rng.integers(-8, 9, Lb).astype(np.float32)


def float_pair(La, Lb, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(La).astype(np.float32), rng.standard_normal(Lb).astype(np.float32)


def rows_of(clips, Lrow, fill=0.0):
    rows = torch.full((len(clips), Lrow), fill, dtype=torch.float32)
    for i, c in enumerate(clips):
        rows[i, :len(c)] = torch.from_numpy(np.asarray(c, np.float32))
    return rows.to("cuda")


def gpu_xcorr(pairs, M, La=None, Lb=None, fill=0.0, lens=None, want_c=True):
    """fd_xcorr_lags on one batch -> (c float64 [B, 2 M + 1] or None, lags int [B]) as host arrays."""
    from flowdec_amd import _lib as L
    lib = L.load()
    B = len(pairs)
    La, Lb = La or max(len(a) for a, _ in pairs), Lb or max(len(b) for _, b in pairs)
    ra, rb = rows_of([a for a, _ in pairs], La, fill), rows_of([b for _, b in pairs], Lb, fill)
    la, lb = lens if lens is not None else ([len(a) for a, _ in pairs], [len(b) for _, b in pairs])
    la, lb = (torch.tensor(v, dtype=torch.int32, device="cuda") for v in (la, lb))
    nws = lib.fd_xcorr_workspace_bytes(B, La, Lb, M)
    assert nws > 0
    ws = torch.empty(nws, dtype=torch.uint8, device="cuda")
    c = torch.full((B, 2 * M + 1), -7.0, dtype=torch.float64, device="cuda") if want_c else None
    lags = torch.full((B,), -77, dtype=torch.int32, device="cuda")
    L.check(lib.fd_xcorr_lags(L.ptr(ra), L.ptr(rb), L.ptr(la), L.ptr(lb), B, La, Lb, M, L.ptr(c), L.ptr(lags), L.ptr(ws), nws, L.stream()))
    torch.cuda.synchronize()
    return (c.cpu().numpy() if want_c else None), lags.cpu().numpy()


@pytest.fixture(scope="module")
def exact():
    """The exact-integer pairs of CASES + OWN_CASES, computed once and never changed."""
    return [integer_pair(La, Lb, d, SEEDS[i]) for i, (La, Lb, M, d) in enumerate(CASES + OWN_CASES)]


@pytest.mark.parametrize("k", range(len(CASES + OWN_CASES)))
def test_exact_integer_data_alone(exact, k):
    from flowdec_amd import align
    La, Lb, M, d = (CASES + OWN_CASES)[k]
    a, b = exact[k]
    want = align.xcorr(a, b, M)
    order = np.sort(want)
    assert align.pick_lag(want) == d and order[-1] > 10 * order[-2] and np.abs(want).max() < 2.0 ** 40
    c, lags = gpu_xcorr([(a, b)], M)
    assert np.array_equal(c[0], want) and lags.tolist() == [d]


@pytest.mark.parametrize("M", [300, 600])
def test_exact_integer_data_as_one_ragged_batch(exact, M):
    from flowdec_amd import align
    pairs = exact[:4]
    c, lags = gpu_xcorr(pairs, M)
    for i, (a, b) in enumerate(pairs):
        assert np.array_equal(c[i], align.xcorr(a, b, M)), i
    assert lags.tolist() == [d for _, _, _, d in CASES[:4]]
    lb, cb = align.lags_batch([torch.from_numpy(a) for a, _ in pairs], [torch.from_numpy(b) for _, b in pairs], M, batch=3, return_xcorr=True)
    assert lb.dtype == np.int64 and lb.tolist() == lags.tolist() and np.array_equal(cb, c)


@pytest.mark.parametrize("k", range(len(CASES)))
def test_float_data_within_the_summation_bound(k):
    from flowdec_amd import align
    La, Lb, M, _ = CASES[k]
    a, b = float_pair(La, Lb, 200 + k)
    want, mass = align.xcorr(a, b, M), align.xcorr(np.abs(a), np.abs(b), M)
    l = np.arange(-M, M + 1)
    terms = np.maximum(0, np.minimum(La, Lb - l) - np.maximum(0, -l))
    c, lags = gpu_xcorr([(a, b)], M)
    err, bound = np.abs(c[0] - want), terms * 2.0 ** -52 * mass
    print(f"La {La} Lb {Lb} M {M}: max |c_gpu - c_ref| / bound = {np.max(err[bound > 0] / bound[bound > 0]):.3g}")
    assert np.all(err <= bound) and lags.tolist() == [align.pick_lag(want)]


def test_batch_invariance_bit_for_bit():
    pairs = [float_pair(4097, 4100, 31), float_pair(700, 1300, 32), float_pair(9001, 8990, 33)]
    M = 600
    alone = [gpu_xcorr([p], M) for p in pairs]
    together = gpu_xcorr(pairs, M)
    backwards = gpu_xcorr(pairs[::-1], M)
    padded = gpu_xcorr(pairs, M, La=40000, Lb=12345)                # the longer rows also add a slice that no clip has
    for i in range(3):
        for c, lags, j in ((together[0], together[1], i), (backwards[0], backwards[1], 2 - i), (padded[0], padded[1], i)):
            assert np.array_equal(c[j].view(np.int64), alone[i][0][0].view(np.int64)) and lags[j] == alone[i][1][0]


def test_poisoned_tails_and_clamped_lengths():
    pairs = [float_pair(4097, 4100, 41), float_pair(700, 1300, 42), float_pair(1000, 1000, 43)]
    M = 600
    zero = gpu_xcorr(pairs, M, La=5000, Lb=4500)
    nan = gpu_xcorr(pairs, M, La=5000, Lb=4500, fill=float("nan"))
    assert np.isfinite(zero[0]).all()
    assert np.array_equal(nan[0].view(np.int64), zero[0].view(np.int64)) and np.array_equal(nan[1], zero[1])
    # lengths beyond the row are clamped to it: the call returns normally and scores the whole rows
    full = [(np.concatenate([a, np.zeros(5000 - len(a), np.float32)]), np.concatenate([b, np.zeros(4500 - len(b), np.float32)])) for a, b in pairs]
    want = gpu_xcorr(full, M)
    got = gpu_xcorr(pairs, M, La=5000, Lb=4500, lens=([5001, 1 << 30, 0x7fffffff], [4501, 99999, 0x7fffffff]))
    assert np.array_equal(got[0].view(np.int64), want[0].view(np.int64)) and np.array_equal(got[1], want[1])
    # negative lengths are empty clips: exact zeros, lag 0
    c, lags = gpu_xcorr(pairs[:1], M, lens=([-5], [4100]))
    assert np.all(c == 0.0) and lags.tolist() == [0]


def test_ties_on_the_device_and_null_c(exact):
    from flowdec_amd import align
    delta = np.zeros(64, np.float32); delta[30] = 1.0
    two = np.zeros(64, np.float32); two[27] = two[33] = 1.0
    near = np.zeros(64, np.float32); near[31] = near[26] = 1.0              # equal maxima at +1 and -4
    silent = np.zeros(500, np.float32)
    pairs = [(silent, silent[:300]), (delta, two), (delta, near)]
    for M in (5, 40):
        c, lags = gpu_xcorr(pairs, M)
        assert lags.tolist() == [0, 3, 1] == [align.best_lag(a, b, M) for a, b in pairs]
        assert np.all(c[0] == 0.0) and c[1][M - 3] == c[1][M + 3] == 1.0 and c[1].sum() == 2.0
    # c = NULL: the same lags
    with_c, without = gpu_xcorr(exact[:4], 600), gpu_xcorr(exact[:4], 600, want_c=False)
    assert without[0] is None and np.array_equal(with_c[1], without[1]) and with_c[1].tolist() == [300, -300, 0, 257]


def test_eval_cli_align_end_to_end(tmp_path, capsys):
    from flowdec_amd import align, eval_cli
    specs = ((int(0.3 * SR), 11, DELAY_H, ADVANCE_Y), (9001, 12, -61, -20))
    lst = make_delayed_triples(tmp_path, specs)
    gpu, host = tmp_path / "gpu.csv", tmp_path / "host.csv"
    flags = ["--batch-files", "2", "--estoi", "--spectral", "--align", "2"]
    r = eval_cli.run(["--triples", str(lst), "--out", str(gpu)] + flags)
    eval_cli.run(["--triples", str(lst), "--out", str(host)] + flags, scorer=eval_cli.HOST_SCORER)
    capsys.readouterr()
    (hg, rg), (hh, rh) = read_csv(gpu), read_csv(host)
    assert hg == hh == list(eval_cli.CSV_HEADER) + ["estoi", "msstft", "mel", "lag_x_hat", "lag_y"]
    assert [row[-2:] for row in rg] == [row[-2:] for row in rh] == [[str(DELAY_H), str(-ADVANCE_Y)], ["-61", "20"]]
    assert r.lags == [("lag_x_hat", -61, DELAY_H, 2), ("lag_y", -ADVANCE_Y, 20, 2)]
    assert float(rg[0][4]) > 35.0 and float(rg[1][4]) > 35.0
    # the same triples cut by hand to the common support, scored without --align: the same kernels see the same samples
    cut_dir = tmp_path / "cut"
    cut_dir.mkdir()
    lines = []
    for i, row in enumerate(rg):
        h, x, y = (eval_cli.load_mono(row[k], SR) for k in (1, 2, 3))
        parts = align.align_triple(h, x, y, int(row[-2]), int(row[-1]))
        assert parts[0].shape == parts[1].shape == parts[2].shape and parts[1].numel() > 8000
        paths = [cut_dir / f"clean_{i}.wav", cut_dir / f"noisy_{i}.wav", cut_dir / f"enh_{i}.wav"]
        for path, s in zip(paths, (parts[1], parts[2], parts[0])):
            write_wav(path, s.numpy(), SR)
        lines.append(" ---> ".join(str(q) for q in paths))
    (cut_dir / "triples_list.txt").write_text("\n".join(lines) + "\n")
    eval_cli.run(["--triples", str(cut_dir / "triples_list.txt"), "--out", str(tmp_path / "cut.csv"), "--batch-files", "2", "--estoi", "--spectral"])
    hc, rc = read_csv(tmp_path / "cut.csv")
    assert hc == hg[:-2] and [row[4:] for row in rc] == [row[4:-2] for row in rg]
