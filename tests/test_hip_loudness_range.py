"""csrc/loudness_range.hip against its yardsticks in flowdec_amd/loudness.py, bit for bit: the true peak of ragged batches and of windows,
the loudness range of synthetic sub-block energies and of a Tech 3342 sequence from audio, batch invariance, the NaN rules, the
streaming meter, other rates, the refusals, loudness_report_batch, and eval_cli --loudness-range --true-peak on the GPU scorer."""
import math
import os

import numpy as np
import pytest
import torch

from loudness_cases import enveloped_noise, loudness_triples, tone
from test_align_cpu import FD_EINVAL, FD_ENOMEM
from test_eval_cpu import read_csv
from test_hip_loudness import feed, raw_rows, same_bits
from test_loudness_range_cpu import TECH_3342, range_energies

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ld():
    from flowdec_amd import loudness
    return loudness


@pytest.fixture(scope="module")
def T():
    from flowdec_amd import _lib as L
    return L.load().fd_true_peak_tile()


@pytest.fixture(scope="module")
def clips(ld, T):
    """One seeded clip per length around the taps and the tile: 1, 2, 2 W - 1, 2 W, T - 1, T, T + 1, 3 T + 7."""
    W = ld.TP_W
    lengths = (1, 2, 2 * W - 1, 2 * W, T - 1, T, T + 1, 3 * T + 7)
    return [(0.3 * np.random.default_rng(40 + k).standard_normal(n)).astype(np.float32) for k, n in enumerate(lengths)]


@pytest.fixture(scope="module")
def peaks(ld, clips):
    """The yardstick's p of every clip, computed once."""
    return [ld.true_peak_lin(x) for x in clips]


def raw_peak(rows, lens, lo=None, hi=None, W=None):
    from flowdec_amd import loudness as ld
    from flowdec_amd import _lib as L
    as_dev = lambda v: None if v is None else torch.tensor(v, dtype=torch.int32).cuda()       # noqa: E731
    B, Lrow = rows.shape
    return ld._true_peak_rows(L.load(), rows, lens, B, Lrow, "cuda", lo=as_dev(lo), hi=as_dev(hi), W=ld.TP_W if W is None else W).cpu().numpy()


def raw_range(Es, Jmax=None, nsub=None):
    """fd_loudness_range on the energies of several clips in ONE call, NaN behind every clip's sub-blocks."""
    from flowdec_amd import loudness as ld
    from flowdec_amd import _lib as L
    Jmax = max(len(E) for E in Es) if Jmax is None else Jmax
    rows = torch.full((len(Es), max(Jmax, 1)), float("nan"), dtype=torch.float64)
    for b, E in enumerate(Es):
        rows[b, :len(E)] = torch.from_numpy(np.ascontiguousarray(E))
    rows = rows[:, :Jmax].contiguous().cuda() if Jmax else None
    n = torch.tensor([len(E) for E in Es] if nsub is None else nsub, dtype=torch.int32).cuda()
    st, counts = ld._range_rows(L.load(), rows, n, len(Es), Jmax, "cuda")
    return st.cpu().numpy(), counts.cpu().numpy()


# ---- true peak -----------------------------------------------------------------------------------------------------------------------------
def test_true_peak_equals_the_yardstick_bit_for_bit(ld, clips, peaks, T):
    got = ld.true_peak_lin_batch(clips, batch=3)
    for k, x in enumerate(clips):
        assert same_bits(got[k], peaks[k]), f"clip {k} ({len(x)} samples): {got[k]!r} vs {peaks[k]!r}"
        assert got[k] >= np.max(np.abs(x))
    assert same_bits(ld.true_peak_batch(clips, batch=8), ld.dbtp_of(np.array(peaks)))
    assert same_bits(ld.true_peak_lin_batch(clips, batch=1), got) and same_bits(ld.true_peak_lin_batch(clips, batch=len(clips)), got)
    for Wo in (1, 5):                                         # another table through the same kernel
        assert same_bits(ld.true_peak_lin_batch(clips[-2:], W=Wo), [ld.true_peak_lin(x, W=Wo) for x in clips[-2:]])
    # a faded tone between the samples: the analytic peak, 3.01 dB above the sample peak
    k = np.arange(4800)
    w = np.minimum(1.0, np.minimum(k + 0.5, 4800 - k - 0.5) / 480.0)
    x = (0.5 * np.sin(2 * np.pi * k / 4 + np.pi / 4) * np.sin(0.5 * np.pi * w) ** 2).astype(np.float32)
    db = ld.true_peak_batch([x])[0]
    assert same_bits(db, ld.true_peak(x)) and abs(db - 20 * math.log10(0.5)) <= 0.05 and db - 20 * math.log10(np.max(np.abs(x))) > 2.9


def test_a_clip_has_the_same_peak_alone_and_anywhere_in_a_ragged_batch(ld, clips, peaks, T):
    x, want = clips[-1], peaks[-1]                            # 3 T + 7 samples
    assert same_bits(raw_peak(*raw_rows([x], len(x)))[0], want)
    others = [clips[k] for k in (5, 2, 6, 4)]
    for pos in (0, 2, 4):
        batch = (others[:pos] + [x] + others[pos:])[:5]
        got = raw_peak(*raw_rows(batch, len(x) + 77))         # NaN behind every clip's end, a row longer than any clip
        assert same_bits(got, [ld.true_peak_lin(c) for c in batch]) and same_bits(got[pos], want), pos
    # a lengths entry beyond L is clamped to L
    rows, lens = raw_rows([x, clips[4]], len(x), fill=0.0)
    lens[0] = len(x) + 5000
    assert same_bits(raw_peak(rows, lens), [want, peaks[4]])


def test_windows_start_and_end_anywhere(ld, clips, T):
    x = clips[-1]
    n, W = len(x), ld.TP_W
    windows = [(0, n), (0, 1), (n - 1, n), (5, T - 3), (T - 3, T + 9), (T, 2 * T), (T + 1, 3 * T + 2), (2 * T + 100, n), (0, T), (n, n), (40, 40),
               (-7, n + 100), (900, 17), (3 * T, n), (W - 1, n - W)]
    rows, lens = raw_rows([x] * len(windows), n + 5)
    got = raw_peak(rows, lens, [w[0] for w in windows], [w[1] for w in windows])
    for (lo, hi), g in zip(windows, got):
        assert same_bits(g, ld.true_peak_lin(x, lo, hi)), (lo, hi)
    assert got[9] == 0.0 and got[10] == 0.0 and got[12] == 0.0 and same_bits(got[11], got[0])
    # different windows on different clips of one call
    batch = [clips[-1], clips[4], clips[6], clips[2]]
    los, his = [T - 1, 3, 0, 22], [2 * T + 1, T - 2, T + 1, 23]
    got = raw_peak(*raw_rows(batch, n), los, his)
    assert same_bits(got, [ld.true_peak_lin(c, a, b) for c, a, b in zip(batch, los, his)])


def test_nan_and_empty_clips_leave_their_neighbours_alone(ld, clips, peaks, T):
    W = ld.TP_W
    x = clips[-1]
    bad_nan, bad_inf, bad_last = x.copy(), x.copy(), x.copy()
    bad_nan[T + 3] = np.nan
    bad_inf[2 * T] = -np.inf
    bad_last[-1] = np.inf
    batch = [clips[5], bad_nan, x, np.zeros(0, np.float32), bad_inf, clips[6], bad_last, np.zeros(300, np.float32)]
    got = ld.true_peak_lin_batch(batch, batch=8)
    assert np.isnan(got).tolist() == [False, True, False, True, True, False, True, False] and got[7] == 0.0
    assert same_bits(got[[0, 2, 5]], [peaks[5], peaks[-1], peaks[6]])
    assert ld.true_peak_batch([np.zeros(300, np.float32)])[0] == -math.inf
    # the bad sample counts exactly when the window reads it: x[lo - W + 1 .. hi + W - 1]
    at = T + 3
    windows = [(0, at - W), (0, at - W + 1), (at + W - 1, len(x)), (at + W, len(x)), (at, at + 1), (2 * T, 3 * T)]
    rows, lens = raw_rows([bad_nan] * len(windows), len(x))
    got = raw_peak(rows, lens, [w[0] for w in windows], [w[1] for w in windows])
    assert np.isnan(got).tolist() == [False, True, True, False, True, False]
    for (lo, hi), g in zip(windows, got):
        assert same_bits(g, ld.true_peak_lin(bad_nan, lo, hi)), (lo, hi)
    # an empty clip in a raw call: NaN, whatever lies in its row
    rows, lens = raw_rows([x, x[:10]], len(x))
    lens[1] = 0
    got = raw_peak(rows, lens)
    assert same_bits(got[0], peaks[-1]) and math.isnan(got[1])


# ---- loudness range ------------------------------------------------------------------------------------------------------------------------
def test_loudness_range_equals_range_of_bit_for_bit(ld):
    Js = (29, 30, 31, 93, 94, 700, 36030)
    Es = [range_energies(J, J) for J in Js]
    quiet = np.full(100, 0.5 * ld.ABS_GATE * 4800.0)                                          # wholly under the absolute gate
    ties = np.concatenate([np.full(200, 4800.0 * 1e-3), np.full(200, 4800.0 * 1e-2)])       # many equal windows
    bad = range_energies(80, 3)
    bad[40] = np.inf
    Es += [quiet, ties, bad, np.zeros(0)]
    want = [ld.range_of(E) for E in Es]
    st, counts = raw_range(Es)                                                                # ragged nsub within ONE call
    for k, (E, (lo, hi, c)) in enumerate(zip(Es, want)):
        assert same_bits(st[k], [lo, hi]) and counts[k].tolist() == c.tolist(), f"clip {k} (J {len(E)}): {st[k]!r} {counts[k]} vs {(lo, hi, c)!r}"
    assert counts[6].tolist()[0] == 36001 and counts[6][2] < counts[6][1] and counts[5][2] < counts[5][1]
    assert st[7].tolist() == [0.0, 0.0] and counts[7].tolist() == [71, 0, 0] and counts[9].tolist() == [51, 0, 0] and counts[10].tolist() == [0, 0, 0]
    assert np.all(np.isnan(st[[0, 9, 10]])) and abs(ld.lra_of(st[8, 0], st[8, 1]) - 10.0) < 1e-9
    # alone, at another position, with an nsub beyond Jmax (clamped) and with fewer sub-blocks than the row holds
    alone, c_alone = raw_range([Es[5]])
    assert same_bits(alone[0], st[5]) and c_alone[0].tolist() == counts[5].tolist()
    st2, c2 = raw_range([Es[3], Es[5], Es[1]], Jmax=700, nsub=[93, 5000, 30])
    assert same_bits(st2, st[[3, 5, 1]]) and np.array_equal(c2, counts[[3, 5, 1]])
    st3, c3 = raw_range([Es[5]], nsub=[94])
    lo, hi, c = ld.range_of(Es[5][:94])
    assert same_bits(st3[0], [lo, hi]) and c3[0].tolist() == c.tolist()
    # power-of-two scaling: the order statistics scale exactly, the counts stay
    st4, c4 = raw_range([Es[5] * 2.0 ** -7])
    assert same_bits(st4[0], st[5] * 2.0 ** -7) and c4[0].tolist() == counts[5].tolist()


def test_tech_3342_sequence_end_to_end_from_audio(ld):
    steps, want = TECH_3342[3]                                # 20 s each at -50, -35, -20, -35, -50 dBFS: 15 LU
    x = tone(1000.0, steps)
    quiet = np.zeros(4 * 48000, np.float32)
    got, counts = ld.loudness_range_batch([x[:100000], x, quiet, x[:3 * 48000 - 1], np.zeros(0, np.float32)], batch=3, return_counts=True)
    host, host_counts = ld.loudness_range(x, return_counts=True)
    assert same_bits(got[1], host) and counts[1].tolist() == host_counts.tolist() and abs(got[1] - want) <= 0.05
    assert math.isnan(got[0]) and got[2] == 0.0 and counts[2].tolist() == [11, 0, 0] and math.isnan(got[3]) and math.isnan(got[4])
    bad = x[:200000].copy()
    bad[150000] = np.nan
    got, counts = ld.loudness_range_batch([bad, x[:200000]], return_counts=True)
    assert math.isnan(got[0]) and counts[0].tolist() == [12, 0, 0] and same_bits(got[1], ld.loudness_range(x[:200000]))


def test_loudness_report_batch_equals_the_three_calls(ld, clips):
    sigs = [enveloped_noise(n, 700 + k) for k, n in enumerate((150003, 24000, 4801, 163200))] + [clips[1], np.zeros(0, np.float32)]
    rep = ld.loudness_report_batch(sigs, batch=4, return_counts=True)
    lufs, c_gate = ld.loudness_batch(sigs, batch=2, return_counts=True)
    lra, c_range = ld.loudness_range_batch(sigs, batch=3, return_counts=True)
    assert same_bits(rep["lufs"], lufs) and same_bits(rep["lra"], lra) and same_bits(rep["dbtp"], ld.true_peak_batch(sigs, batch=5))
    assert np.array_equal(rep["lufs_counts"], c_gate) and np.array_equal(rep["lra_counts"], c_range)
    assert math.isfinite(rep["lra"][0]) and math.isfinite(rep["lra"][3]) and math.isnan(rep["lra"][1]) and math.isnan(rep["dbtp"][5])
    assert same_bits(rep["lra"][0], ld.loudness_range(sigs[0])) and same_bits(rep["lufs"][0], ld.integrated_loudness(sigs[0]))
    # a file of two channels: the energies added and gated once, the larger peak
    lufs2, dbtp2 = ld.file_level_batch([[sigs[1], sigs[1]], [sigs[1]], [sigs[1] * np.float32(0.5), sigs[1]]])
    assert same_bits([lufs2[0], dbtp2[0]], ld.file_level([sigs[1], sigs[1]])) and same_bits(lufs2[1], lufs[1]) and same_bits(dbtp2[[0, 1, 2]], [rep["dbtp"][1]] * 3)
    assert abs((lufs2[0] - lufs2[1]) - 10 * math.log10(2.0)) < 1e-9


# ---- the meter -----------------------------------------------------------------------------------------------------------------------------
def test_streaming_meter_equals_the_one_shot_calls_after_every_push(ld):
    x = enveloped_noise(150001, 910)                   # 3.1 s: 31 sub-blocks, so the range exists at the end
    q = np.round(x[:30000] * 32767.0).astype(np.int16)
    xq = q.astype(np.float32) / np.float32(32768.0)
    E_all = ld.kweight_energies(x)

    def check(meter, s, E, n):
        """After n samples: both answers are the one-shot calls' on s[:n], and asking twice changes nothing."""
        want_p = ld.dbtp_of(ld.true_peak_lin(s[:n]))
        lo, hi, counts = ld.range_of(E[:n // 4800])
        for _ in range(2):
            assert same_bits(meter.true_peak(), want_p), n
            got, got_counts = meter.loudness_range(return_counts=True)
            assert same_bits(got, ld.lra_of(lo, hi)) and got_counts.tolist() == counts.tolist(), n

    meter, asked, n, k = ld.LoudnessMeter(), ld.LoudnessMeter(), 0, 0
    assert math.isnan(meter.true_peak()) and math.isnan(meter.loudness_range())
    sizes = [1] * 30 + [23, 4799, 4800, 7001, 1]      # a sample at a time across W and 2 W - 1, then the cycle
    while n < len(x):
        size = sizes[k] if k < len(sizes) else sizes[30 + k % 5]
        meter.push(x[n:n + size])
        asked.push(x[n:n + size])
        n, k = min(n + size, len(x)), k + 1
        check(asked, x, E_all, n)
    # the meter that was never asked answers the same, and the one-shot device call agrees
    assert same_bits(meter.true_peak(), asked.true_peak()) and same_bits(meter.loudness_range(), asked.loudness_range())
    assert math.isfinite(meter.loudness_range()) and same_bits(meter.true_peak(), ld.true_peak_batch([x])[0])
    assert same_bits(meter.loudness_range(), ld.loudness_range_batch([x])[0]) and same_bits(meter.integrated(), ld.integrated_loudness(x))
    whole = ld.LoudnessMeter()
    whole.push(torch.from_numpy(x).cuda())
    assert same_bits(whole.true_peak(), meter.true_peak()) and same_bits(whole.loudness_range(), meter.loudness_range())
    # an int16 feed
    m16, n = ld.LoudnessMeter(), 0
    for size in (23, 4799, 1, 7001, 4800, 7001, 7001):
        m16.push(q[n:n + size])
        n = min(n + size, len(q))
        check(m16, xq, ld.kweight_energies(xq), n)
    # a NaN sample is kept: in the tail first, then among the committed positions
    bad = x[:9000].copy()
    bad[4000] = np.nan
    mb = feed(ld.LoudnessMeter(), bad[:3990], (1000,))
    assert math.isfinite(mb.true_peak())
    mb.push(bad[3990:4005])
    assert math.isnan(mb.true_peak())
    feed(mb, bad[4005:], (2000,))
    assert math.isnan(mb.true_peak()) and math.isnan(ld.true_peak(bad))


@pytest.mark.parametrize("sr", [16000, 44100])
def test_other_rates_are_resampled_on_the_device_first(ld, sr):
    from flowdec_amd.resample import resample_device
    x = enveloped_noise(int(3.3 * sr) + 17, 960 + sr % 7)
    up = resample_device(torch.from_numpy(x).cuda(), sr, 48000, lowpass_filter_width=64).cpu().numpy()
    rep = ld.loudness_report_batch([x, x[:sr // 2]], sr=sr)
    assert same_bits(rep["dbtp"][0], ld.dbtp_of(ld.true_peak_lin(up))) and same_bits(rep["lra"][0], ld.loudness_range(up))
    assert math.isfinite(rep["lra"][0]) and math.isnan(rep["lra"][1]) and math.isfinite(rep["dbtp"][1])
    # the host resampler differs by float32 rounding of the FIR only
    assert abs(rep["dbtp"][0] - ld.true_peak(x, sr)) < 1e-4 and abs(rep["lra"][0] - ld.loudness_range(x, sr)) < 1e-4
    with pytest.raises(ValueError, match="cap"):
        ld.true_peak_batch([x], sr=47999)


# ---- refusals and the command line -----------------------------------------------------------------------------------------------------------
def test_refusals_leave_a_message_and_the_outputs_untouched(ld):
    from flowdec_amd import _lib as L
    lib = L.load()
    rows, lens = raw_rows([enveloped_noise(5000, 1)], 5000)
    taps = ld._tp_taps(ld.TP_W, "cuda")
    nws = lib.fd_true_peak_workspace_bytes(1, 5000)
    ws = torch.empty(nws, dtype=torch.uint8, device="cuda")
    p = torch.full((1,), 7.0, dtype=torch.float64, device="cuda")
    err = lambda: lib.fd_last_error().decode()                # noqa: E731
    peak = lambda x=rows, W=ld.TP_W, taps=taps, n=nws, B=1: lib.fd_true_peak(L.ptr(x), L.ptr(lens), B, 5000, None, None, L.ptr(taps), W, L.ptr(p), L.ptr(ws), n, L.stream())   # noqa: E731
    assert peak(W=0) == FD_EINVAL and "W 0" in err()
    assert peak(W=257) == FD_EINVAL and "W 257" in err()
    assert peak(x=None) == FD_EINVAL and "null pointer" in err()
    assert peak(taps=None) == FD_EINVAL and "taps" in err()
    assert peak(B=0) == FD_EINVAL and "B 0" in err()
    assert peak(n=nws - 1) == FD_ENOMEM and "fd_true_peak" in err() and "workspace" in err()
    E = torch.from_numpy(range_energies(40, 1)).reshape(1, -1).cuda()
    nsub = torch.tensor([40], dtype=torch.int32).cuda()
    st = torch.full((1, 2), 7.0, dtype=torch.float64, device="cuda")
    counts = torch.full((1, 3), -1, dtype=torch.int32, device="cuda")
    nwr = lib.fd_loudness_range_workspace_bytes(1, 40)
    wr = torch.empty(nwr, dtype=torch.uint8, device="cuda")
    rng = lambda E=E, J=40, st=st, n=nwr: lib.fd_loudness_range(L.ptr(E), L.ptr(nsub), 1, J, L.ptr(st), L.ptr(counts), L.ptr(wr), n, L.stream())   # noqa: E731
    assert rng(E=None) == FD_EINVAL and "null pointer" in err()
    assert rng(st=None) == FD_EINVAL and "null pointer" in err()
    assert rng(J=-1) == FD_EINVAL and "Jmax -1" in err()
    assert rng(n=nwr - 1) == FD_ENOMEM and "fd_loudness_range" in err() and "workspace" in err()
    torch.cuda.synchronize()
    assert p.item() == 7.0 and st.tolist() == [[7.0, 7.0]] and counts.tolist() == [[-1, -1, -1]]
    # and the same buffers are written by calls that are taken
    assert peak() == 0 and rng() == 0
    torch.cuda.synchronize()
    assert p.item() != 7.0 and counts[0].tolist() == [11, 11, counts[0, 2].item()] and st[0, 0].item() != 7.0
    with pytest.raises(ValueError):
        ld.true_peak_lin_batch([np.zeros(10, np.float32)], W=0)


def test_enhance_cli_target_lufs_one_process_and_two_workers(ld, tmp_path, capsys):
    """A small random-weight flow model (the preset of the other command-line GPU tests) over two files of one bucket, a file that runs in
    rows (--chunk-seconds) and a file at another rate: every written file re-measures at the target on the host yardstick (or, where the
    ceiling capped the gain, peaks at the ceiling), loudness.csv holds what was measured, and `--gpus 2 --share-gpu` writes the same bytes.
    (The models take one channel, so the several-channel rule is checked on the library: test_loudness_report_batch_equals_the_three_calls.)"""
    from flowdec_amd import enhance_cli
    from flowdec_amd.audio import load_wav
    from test_hip_multigpu import _ckpt, _launch, _wavs, _write_corpus
    ckpt = _ckpt(tmp_path)
    spec = [("a", 30000, 48000, 1), ("f", 20000, 48000, 1), ("g", 23000, 48000, 1), ("h", 12000, 16000, 1)]
    _write_corpus(tmp_path / "in", spec)
    common = ["--ckpt", ckpt, "--files", str(tmp_path / "in"), "--N", "2", "--solver", "midpoint", "--batch-files", "4", "--rng", "native", "--seed", "3",
              "--chunk-seconds", "0.6", "--max-seconds", "1", "--rtf"]
    plain = enhance_cli.run(common + ["--outdir", str(tmp_path / "p1")])
    one = enhance_cli.run(common + ["--outdir", str(tmp_path / "o1"), "--target-lufs", "-23"])
    out = capsys.readouterr().out
    assert plain.n_done == one.n_done == 4 and "Long file:" in out
    assert sorted(os.listdir(tmp_path / "o1")) == sorted(os.listdir(tmp_path / "p1") + ["loudness.csv"])
    lines = (tmp_path / "o1" / "loudness.csv").read_text().splitlines()
    assert lines[0] == "name,lufs,dbtp,gain_db,limited" and sorted(l.split(",")[0] for l in lines[1:]) == sorted(f"{s[0]}.wav" for s in spec)
    for line in lines[1:]:
        name, lufs, dbtp, gain, limited = line.split(",")
        before = list(load_wav(str(tmp_path / "p1" / name))[0].numpy())
        after = list(load_wav(str(tmp_path / "o1" / name))[0].numpy())
        assert len(before) == 1
        want_lufs, want_dbtp = ld.file_level(before)                 # the host yardstick on the plain run's file: what the GPU measured
        assert same_bits([float(lufs), float(dbtp)], [want_lufs, want_dbtp]), name
        g, lim = ld.output_gain(want_lufs, want_dbtp, -23.0, -1.0)
        assert float(gain) == g and limited == str(int(lim))
        assert all(np.array_equal(a, b * np.float32(10.0 ** (g / 20.0))) for a, b in zip(after, before))
        got_lufs, got_dbtp = ld.file_level(after)
        print(name, "was", want_lufs, "LUFS", want_dbtp, "dBTP; gain", g, "-> re-measured", got_lufs, got_dbtp)
        # one float32 multiply per sample and the factor's own rounding: under 1.1e-6 dB
        assert abs(got_dbtp - -1.0) <= 1e-4 if lim else abs(got_lufs - -23.0) <= 1e-4
    child = _launch(common + ["--outdir", str(tmp_path / "o2"), "--target-lufs", "-23", "--gpus", "2", "--share-gpu"])
    assert child.returncode == 0, (child.stdout + child.stderr)[-3000:]
    assert sorted(os.listdir(tmp_path / "o1")) == sorted(os.listdir(tmp_path / "o2"))                # no part file, no manifest
    assert _wavs(tmp_path / "o1") == _wavs(tmp_path / "o2")
    assert (tmp_path / "o1" / "loudness.csv").read_bytes() == (tmp_path / "o2" / "loudness.csv").read_bytes()


def test_eval_cli_on_the_gpu(ld, tmp_path, capsys):
    from flowdec_amd import eval_cli
    from flowdec_amd.audio import save_wav
    lst, sigs = loudness_triples(tmp_path)
    long = tone(1000.0, [(-20, 2.0), (-32, 2.0)])          # a seventh triple long enough for a range
    noisy = long + (0.001 * np.random.default_rng(8).standard_normal(len(long))).astype(np.float32)
    paths = [tmp_path / n for n in ("clean_long.wav", "noisy_long.wav", "enh_long.wav")]
    for p, s in zip(paths, (long, noisy, long * np.float32(0.5))):
        save_wav(str(p), torch.from_numpy(s), 48000)
    with open(lst, "a") as f:
        f.write(" ---> ".join(str(p) for p in paths) + "\n")
    G, H = eval_cli.GPU_SCORER, eval_cli.HOST_SCORER
    outs = {}
    flags = ["--loudness", "--loudness-range", "--true-peak"]
    for name, scorer, fl in (("gpu", G, flags), ("host", H, flags), ("plain", G, []),
                             ("before", eval_cli.Scorer(G.si_sxr, G.logspec, G.estoi, G.spectral, G.align, G.align_frac, G.shift, G.loudness, G.segsnr), [])):
        out = tmp_path / f"{name}.csv"
        res = eval_cli.run(["--triples", str(lst), "--out", str(out), "--batch-files", "4"] + fl, scorer=scorer)
        assert res.exit_code == 0 and res.n_scored == 7
        outs[name] = (out, capsys.readouterr(), res)
    hg, rg = read_csv(outs["gpu"][0])
    hh, rh = read_csv(outs["host"][0])
    assert hg == hh and tuple(hg[-9:]) == eval_cli.LUFS_NAMES + eval_cli.LRA_NAMES + eval_cli.DBTP_NAMES
    # the range and the peak are the yardsticks' bits, so their text is the host scorer's
    assert [r[-6:] for r in rg] == [r[-6:] for r in rh]
    assert all(r[-6:-3] == ["nan"] * 3 for r in rg[:6]) and all(math.isfinite(float(v)) for v in rg[6][-6:])
    assert abs(float(rg[6][-6]) - float(rg[6][-5])) < 1e-6 and float(rg[6][-5]) > 1.0 and abs((float(rg[6][-2]) - float(rg[6][-3])) - 20 * math.log10(2.0)) < 1e-6
    assert [c for _, _, c in outs["gpu"][2].loudness_range] == [1, 1, 1] and [c for _, _, c in outs["gpu"][2].true_peak] == [7, 7, 7]
    # without the flags: every byte is what a scorer without the new fields writes
    assert outs["plain"][0].read_bytes() == outs["before"][0].read_bytes()
    assert outs["plain"][1].out.replace("plain.csv", "x.csv") == outs["before"][1].out.replace("before.csv", "x.csv") and "dbtp" not in outs["plain"][1].out
