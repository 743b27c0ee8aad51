"""flowdec_amd/loudness.py on the host: the yardsticks of csrc/loudness_range.hip -- loudness range against the tone sequences of EBU Tech
3342 and a literal transcription, true peak against analytic tone peaks and a literal double loop, the output gain of EBU R 128 by hand
values, the several-channel rule -- and eval_cli --loudness-range / --true-peak on the host scorer.  No GPU."""
import ctypes as C
import math
import os
import types

import numpy as np
import pytest

from loudness_cases import SR, loudness_triples, tone
from test_align_cpu import FD_EINVAL, FD_ENOMEM
from test_eval_cpu import read_csv
from test_loudness_cpu import run_cli


@pytest.fixture(scope="module")
def ld():
    from flowdec_amd import loudness
    return loudness


# ---- loudness range ------------------------------------------------------------------------------------------------------------------------
def literal_range(E, ld):
    """Steps a to e of loudness.py written out with Python floats, loops and np.sort -> (st_lo, st_hi, counts)."""
    E = [float(v) for v in E]
    J = len(E)
    if J < 30:
        return math.nan, math.nan, [0, 0, 0]
    st = []
    for j in range(J - 29):
        a = E[j] + E[j + 1]
        for k in range(2, 30):
            a = a + E[j + k]
        st.append(a / 144000.0)
    if not all(math.isfinite(s) for s in st):
        return math.nan, math.nan, [len(st), 0, 0]
    keep1 = [s > ld.ABS_GATE for s in st]
    n1 = sum(keep1)
    if n1 == 0:
        return 0.0, 0.0, [len(st), 0, 0]
    lanes = [0.0] * 64
    for j, s in enumerate(st):
        lanes[j % 64] = lanes[j % 64] + (s if keep1[j] else 0.0)
    total = lanes[0]
    for l in range(1, 64):
        total = total + lanes[l]
    thr = 0.01 * (total / n1)
    kept = np.sort(np.array([s for s, k in zip(st, keep1) if k and s > thr], np.float64))
    m = len(kept)
    return kept[((m - 1) * 10 + 50) // 100], kept[((m - 1) * 95 + 50) // 100], [len(st), n1, m]


def same_bits(a, b):
    return np.array_equal(np.array(a, np.float64).view(np.uint64), np.array(b, np.float64).view(np.uint64))


def range_energies(J: int, seed: int) -> np.ndarray:
    """Random positive sub-block energies whose level holds for 3.5 s at a time, the levels spread over 40 dB and jittered by 2 dB: the
    short-term windows then differ by more than 20 LU, so the relative gate removes some of a longer input."""
    rng = np.random.default_rng(seed)
    level = np.repeat(rng.uniform(-5.0, -1.0, J // 35 + 1), 35)[:J] + rng.uniform(-0.2, 0.2, J)
    return 4800.0 * 10.0 ** level


TECH_3342 = [([(-20, 20), (-30, 20)], 10.0), ([(-20, 20), (-15, 20)], 5.0), ([(-40, 20), (-20, 20)], 20.0),
             ([(-50, 20), (-35, 20), (-20, 20), (-35, 20), (-50, 20)], 15.0)]


@pytest.mark.parametrize("steps,want", TECH_3342, ids=["10LU", "5LU", "20LU", "15LU"])
def test_conformance_tech_3342(ld, steps, want):
    """EBU Tech 3342's tone sequences (1 kHz sines at the stated dBFS levels): the standard allows +-1 LU; the definition read 10.000,
    5.000, 20.000 and 15.000, and 0.05 LU leaves room for another legal summation order in this test's own arithmetic."""
    got, counts = ld.loudness_range(tone(1000.0, steps), return_counts=True)
    print("Tech 3342", steps, "reads", got, "LU, counts", counts)
    assert abs(got - want) <= 0.05
    assert counts[0] == sum(s for _, s in steps) * 10 - 29 and counts[0] >= counts[1] >= counts[2] >= 1


@pytest.mark.parametrize("J", [29, 30, 31, 93, 94, 700])
def test_range_of_is_the_literal_transcription(ld, J):
    """93 and 94 sub-blocks give 64 and 65 windows, where the lane sum wraps."""
    E = range_energies(J, J)
    lo, hi, counts = ld.range_of(E)
    wlo, whi, wcounts = literal_range(E, ld)
    assert same_bits([lo, hi], [wlo, whi]) and list(counts) == wcounts and counts.dtype == np.int32
    if J < 30:
        assert math.isnan(lo) and math.isnan(hi) and list(counts) == [0, 0, 0] and math.isnan(ld.lra_of(lo, hi))
    else:
        assert counts[0] == J - 29 and hi >= lo > 0 and ld.lra_of(lo, hi) == 10 * np.log10(hi) - 10 * np.log10(lo) >= 0
        i_lo, i_hi = ld.range_ranks(int(counts[2]))
        assert (i_lo, i_hi) == (((counts[2] - 1) * 10 + 50) // 100, ((counts[2] - 1) * 95 + 50) // 100) and 0 <= i_lo <= i_hi < counts[2]
    if J == 700:
        assert counts[2] < counts[1] == counts[0]          # the relative gate did something


def test_range_edge_cases(ld):
    rng = np.random.default_rng(5)
    # every window under the absolute gate: 0.0 LU
    E = np.full(100, 0.5 * ld.ABS_GATE * 4800.0)
    lo, hi, counts = ld.range_of(E)
    assert lo == 0.0 and hi == 0.0 and list(counts) == [71, 0, 0] and ld.lra_of(lo, hi) == 0.0
    assert ld.loudness_range(np.zeros(4 * SR, np.float32)) == 0.0 and math.isnan(ld.loudness_range(np.zeros(3 * SR - 1, np.float32)))
    # a non-finite energy: NaN and (windows, 0, 0), whichever kind
    for bad in (np.nan, np.inf):
        E = 4800.0 * 10.0 ** rng.uniform(-4, -2, 80)
        E[40] = bad
        lo, hi, counts = ld.range_of(E)
        assert math.isnan(lo) and math.isnan(hi) and list(counts) == [51, 0, 0] and math.isnan(ld.lra_of(lo, hi))
    # ties: many equal windows (two plateaus and the ramp between them); selection by value cannot depend on how ties are ordered
    E = np.concatenate([np.full(200, 4800.0 * 1e-3), np.full(200, 4800.0 * 1e-2)])
    lo, hi, counts = ld.range_of(E)
    wlo, whi, wcounts = literal_range(E, ld)
    assert same_bits([lo, hi], [wlo, whi]) and list(counts) == wcounts == [371, 371, 371]
    assert abs(ld.lra_of(lo, hi) - 10.0) < 1e-9
    # scaling E by a power of two scales every window, the threshold and both order statistics exactly and keeps the counts (all
    # windows stay far above the absolute gate); LRA = 10 log10(hi) - 10 log10(lo) then agrees to the rounding of its two logarithms
    # (each within an ulp of a value under 100: 1.4e-14), which is not nothing: 3.6e-15 was seen
    E = 4800.0 * 10.0 ** rng.uniform(-3.0, -1.0, 700)
    a, b = ld.range_of(E), ld.range_of(E * 2.0 ** -7)
    assert same_bits([a[0] * 2.0 ** -7, a[1] * 2.0 ** -7], [b[0], b[1]]) and np.array_equal(a[2], b[2])
    print("LRA", ld.lra_of(a[0], a[1]), "scaled by 2^-7", ld.lra_of(b[0], b[1]))
    assert abs(ld.lra_of(a[0], a[1]) - ld.lra_of(b[0], b[1])) <= 1e-13
    assert ld.lra_of(np.array([0.0, 1.0]), np.array([0.0, 10.0])).tolist() == [0.0, 10.0]


# ---- true peak -----------------------------------------------------------------------------------------------------------------------------
def literal_peak(x, ld, lo=0, hi=None, W=None):
    """The definition as a double loop over positions and phases, with Python floats."""
    W = ld.TP_W if W is None else W
    H = ld.align.frac_bank(4, W).tolist()
    xs = [float(v) for v in np.asarray(x, np.float32)]
    n = len(xs)
    if n == 0:
        return math.nan
    lo = min(max(lo, 0), n)
    hi = min(max(n if hi is None else hi, lo), n)
    p, bad = 0.0, False
    for pos in range(lo, hi):
        for j in range(4):
            acc = 0.0
            for t in range(2 * W):
                m = pos + t - W + 1
                v = xs[m] if 0 <= m < n else 0.0
                acc = acc + v * H[j][t]
            if not math.isfinite(acc):
                bad = True
            p = max(p, abs(acc))
    return math.nan if bad else p


def faded_tone(period: int, phase_deg: float, amplitude: float, n: int = 4800, fade: int = 480, sr_fade: bool = True):
    """amplitude * sin(2 pi k / period + phase) under a raised-cosine fade of `fade` samples (10 ms) at both ends."""
    k = np.arange(n)
    x = amplitude * np.sin(2 * np.pi * k / period + np.deg2rad(phase_deg))
    w = np.ones(n)
    if sr_fade:
        r = 0.5 * (1.0 - np.cos(np.pi * (np.arange(fade) + 0.5) / fade))
        w[:fade], w[-fade:] = r, r[::-1]
    return (x * w).astype(np.float32)


TP_TONES = [(4, 0.0, 0.5), (4, 45.0, 0.5), (6, 60.0, 0.5), (8, 67.5, 0.5), (4, 45.0, 1.41)]


@pytest.mark.parametrize("period,phase,amp", TP_TONES, ids=["fs4-0", "fs4-45", "fs6-60", "fs8-67.5", "fs4-45-over"])
def test_true_peak_of_faded_tones_is_analytic(ld, period, phase, amp):
    """EBU Tech 3341 allows +0.2 / -0.4 dB; the definition at W = 12 read within 0.005 dB of 20 log10(amplitude)."""
    x = faded_tone(period, phase, amp)
    got = ld.true_peak(x)
    print("tone fs/%d at %g deg, amplitude %g: %.6f dBTP, analytic %.6f" % (period, phase, amp, got, 20 * math.log10(amp)))
    assert abs(got - 20 * math.log10(amp)) <= 0.05
    assert ld.dbtp_of(ld.true_peak_lin(x)) == got and ld.TP_W == 12 and ld.TP_Q == 4
    if (period, phase) == (4, 45.0):
        sample_peak = 20 * math.log10(float(np.max(np.abs(x))))
        assert abs((got - sample_peak) - 3.0103) <= 0.05          # the point of the measure: the samples sit 3.01 dB under the peak


def test_true_peak_unfaded_tone_is_the_literal_loop(ld):
    """Without the fade the zero-extended edges ring (+0.1 to +0.7 dB were seen): the definition at work, so only the value is checked."""
    x = faded_tone(4, 45.0, 0.5, n=600, sr_fade=False)
    got = ld.true_peak_lin(x)
    assert same_bits(got, literal_peak(x, ld))
    print("unfaded fs/4 45 deg reads", ld.dbtp_of(got) - 20 * math.log10(0.5), "dB over the analytic peak")
    assert ld.dbtp_of(got) >= 20 * math.log10(0.5) - 0.05


@pytest.mark.parametrize("n", [1, 2, 23, 24, 1000])
def test_true_peak_is_the_literal_loop(ld, n):
    W = ld.TP_W
    assert (2 * W - 1, 2 * W) == (23, 24)
    x = (0.5 * np.random.default_rng(n).standard_normal(n)).astype(np.float32)
    assert same_bits(ld.true_peak_lin(x), literal_peak(x, ld))
    assert ld.true_peak_lin(x) >= np.max(np.abs(x))                  # row 0 is the unit impulse
    windows = [(0, n), (0, n // 2), (n // 2, n), (n // 3, 2 * n // 3), (n - 1, n), (0, 1), (-5, n + 9), (n, n), (3, 3), (7, 2)]
    for lo, hi in windows:
        assert same_bits(ld.true_peak_lin(x, lo, hi), literal_peak(x, ld, lo, hi)), (lo, hi)
    assert ld.true_peak_lin(x, n, n) == 0.0                          # an empty window of a clip that is not empty
    # the maximum over windows that cover the clip is the clip's
    cuts = sorted({0, n // 3, n // 2, n})
    assert same_bits(max(ld.true_peak_lin(x, a, b) for a, b in zip(cuts[:-1], cuts[1:])), ld.true_peak_lin(x))
    if n == 1000:
        for Wo in (1, 5):
            assert same_bits(ld.true_peak_lin(x, W=Wo), literal_peak(x, ld, W=Wo))


def test_true_peak_nan_inf_and_empty(ld):
    W = ld.TP_W
    assert math.isnan(ld.true_peak_lin(np.zeros(0, np.float32))) and math.isnan(ld.true_peak(np.zeros(0, np.float32)))
    assert ld.true_peak_lin(np.zeros(50, np.float32)) == 0.0 and ld.true_peak(np.zeros(50, np.float32)) == -math.inf
    x = (0.1 * np.random.default_rng(1).standard_normal(300)).astype(np.float32)
    for bad in (np.nan, np.inf, -np.inf):
        y = x.copy()
        y[100] = bad
        assert math.isnan(ld.true_peak_lin(y)) and math.isnan(literal_peak(y, ld)) and math.isnan(ld.true_peak(y))
        # a window reads the samples lo - W + 1 .. hi + W - 1: the bad sample counts exactly when it is among them
        for lo, hi in ((0, 100 - W), (0, 100 - W + 1), (100 + W - 1, 300), (100 + W, 300), (100, 101)):
            got, want = ld.true_peak_lin(y, lo, hi), literal_peak(y, ld, lo, hi)
            assert same_bits(got, want), (bad, lo, hi)
            assert math.isnan(got) == (lo - W + 1 <= 100 <= hi + W - 1)
    with pytest.raises(ValueError):
        ld.true_peak_lin(x, W=0)
    with pytest.raises(TypeError):
        ld.true_peak_lin(x.astype(np.float64))
    with pytest.raises(ValueError, match="cap"):
        ld.true_peak(x, 47999)
    assert ld.dbtp_of(0.0) == -math.inf and ld.dbtp_of(1.0) == 0.0 and math.isnan(ld.dbtp_of(math.nan))
    # another rate goes through the resampler in front, as integrated_loudness does
    t16 = faded_tone(8, 0.0, 0.5, n=1600, fade=160)
    assert abs(ld.true_peak(t16, 16000) - 20 * math.log10(0.5)) <= 0.05
    assert np.array_equal(ld.host_true_peak([x, t16[:300]]), [ld.true_peak(x), ld.true_peak(t16[:300])])


# ---- output gain ---------------------------------------------------------------------------------------------------------------------------
def test_output_gain_by_hand(ld):
    assert ld.output_gain(-20.0, -10.0, -23.0) == (-3.0, False)
    assert ld.output_gain(-30.0, -10.0, -16.0) == (14.0, False)                   # no ceiling, no cap
    assert ld.output_gain(-30.0, -10.0, -16.0, -1.0) == (9.0, True)               # -10 + 14 > -1: the cap brings the peak to -1 dBTP
    assert ld.output_gain(-24.0, -9.0, -16.0, -1.0) == (8.0, False)               # -9 + 8 = -1 exactly: at the ceiling, not over it
    assert ld.output_gain(-24.0, -8.5, -16.0, -1.0) == (7.5, True)
    assert ld.output_gain(-20.0, -0.5, -20.0, -1.0) == (-0.5, True)               # 0 dB asked, the ceiling still holds
    for lufs, dbtp in ((math.nan, -3.0), (-math.inf, -math.inf), (-20.0, math.nan), (math.inf, 0.0)):
        assert ld.output_gain(lufs, dbtp, -23.0, -1.0) == (None, False)
    x = tone(1000.0, [(-20, 2.0)])
    lufs, dbtp = ld.integrated_loudness(x), ld.true_peak(x)
    y, g, limited = ld.normalize_loudness(x, lufs, dbtp, -23.0, -1.0)
    assert g == -23.0 - lufs and not limited and y.dtype == np.float32 and np.array_equal(y, x * np.float32(10.0 ** (g / 20.0)))
    # one float32 multiply per sample is 2^-24 relative on the samples, the factor's own rounding another 2^-24: under 1.1e-6 dB
    print("re-measured", ld.integrated_loudness(y), "after a gain of", g)
    assert abs(ld.integrated_loudness(y) - -23.0) <= 1e-4
    y, g, limited = ld.normalize_loudness(x, lufs, dbtp, -3.0, -1.0)              # the ceiling engages: the peak lands on it
    assert limited and g == -1.0 - dbtp and abs(ld.true_peak(y) - -1.0) <= 1e-4
    same, g, limited = ld.normalize_loudness(x[:100], ld.integrated_loudness(x[:100]), ld.true_peak(x[:100]), -23.0, -1.0)
    assert same is not None and g is None and not limited and np.array_equal(same, x[:100])


def test_files_of_several_channels(ld):
    """Two channels of the same tone read 10 log10(2) = 3.01 LU above one; the true peak is the maximum over the channels."""
    x = tone(1000.0, [(-20, 3.0)])
    quiet = (x * np.float32(0.25)).astype(np.float32)
    one, _ = ld.file_level([x])
    two, peak2 = ld.file_level([x, x])
    assert one == ld.integrated_loudness(x) and abs((two - one) - 10 * math.log10(2.0)) <= 1e-9
    _, peak = ld.file_level([quiet, x])
    assert peak == peak2 == ld.true_peak(x) > ld.true_peak(quiet)
    E = ld.kweight_energies(x)
    assert np.array_equal(ld.file_energies([E, E, E]), (E + E) + E)
    bad = x.copy()
    bad[5] = np.nan
    assert math.isnan(ld.file_level([x, bad])[1])
    with pytest.raises(ValueError):
        ld.file_energies([E, E[:-1]])


# ---- eval_cli ------------------------------------------------------------------------------------------------------------------------------
def test_eval_cli_range_and_peak_columns(ld, tmp_path, capsys):
    from flowdec_amd import eval_cli
    lst, sigs = loudness_triples(tmp_path)
    H = eval_cli.HOST_SCORER
    base, out_base = run_cli(tmp_path, lst, "base.csv", [], H)
    capsys.readouterr()
    both, out_both = run_cli(tmp_path, lst, "both.csv", ["--loudness-range", "--true-peak"], H)
    cap_both = capsys.readouterr()
    full, out_full = run_cli(tmp_path, lst, "full.csv", ["--estoi", "--align", "1", "--match-loudness", "--true-peak", "--loudness-range"], H)
    capsys.readouterr()
    peak, out_peak = run_cli(tmp_path, lst, "peak.csv", ["--true-peak"], H)
    capsys.readouterr()
    h0, r0 = read_csv(out_base)
    h1, r1 = read_csv(out_both)
    h2, r2 = read_csv(out_full)
    h3, r3 = read_csv(out_peak)
    assert eval_cli.LRA_NAMES == ("lra_x_hat", "lra_x", "lra_y") and eval_cli.DBTP_NAMES == ("dbtp_x_hat", "dbtp_x", "dbtp_y")
    assert tuple(h1) == eval_cli.CSV_HEADER + eval_cli.LRA_NAMES + eval_cli.DBTP_NAMES and tuple(h3) == eval_cli.CSV_HEADER + eval_cli.DBTP_NAMES
    assert tuple(h2) == eval_cli.CSV_HEADER + ("estoi",) + eval_cli.LUFS_NAMES + eval_cli.LRA_NAMES + eval_cli.DBTP_NAMES + ("lag_x_hat", "lag_y")
    # no other column is touched; the new ones are the yardsticks' readings of the signals as scored (all under 3 s: no range)
    assert [r[:8] for r in r1] == r0 == [r[:8] for r in r3]
    assert [r[8:11] for r in r1] == [["nan"] * 3 for _ in sigs]
    want = [[eval_cli.fmt(ld.true_peak(s)) for s in t] for t in sigs]
    assert [r[11:] for r in r1] == want == [r[8:] for r in r3]
    # with --match-loudness the columns still report the state before the scaling (lag 0 here: the signals are scored whole)
    assert [r[15:18] for r in r2] == want and [r[-2:] for r in r2] == [["0", "0"]] * len(sigs)
    assert [n for n, _, _ in both.true_peak] == list(eval_cli.DBTP_NAMES) and all(c == 6 for _, _, c in both.true_peak)
    assert [n for n, _, _ in both.loudness_range] == list(eval_cli.LRA_NAMES) and all(c == 0 for _, _, c in both.loudness_range)
    assert base.true_peak == [] and base.loudness_range == [] and peak.loudness_range == [] and both.loudness == []
    assert "dbtp_x_hat   mean = " in cap_both.out and "lra_x        mean = nan  over 0 finite rows" in cap_both.out
    assert cap_both.out.index("lra_x_hat") < cap_both.out.index("dbtp_x_hat")


@pytest.mark.filterwarnings("ignore::RuntimeWarning")      # x_hat is x at half the level: the host SI-SAR divides by a zero artefact
def test_eval_cli_loudness_range_of_a_long_triple(ld, tmp_path, capsys):
    import torch
    from flowdec_amd import eval_cli
    from flowdec_amd.audio import save_wav
    x = tone(1000.0, [(-20, 2.5), (-30, 2.5)])
    h = (x * np.float32(0.5)).astype(np.float32)
    y = x + (0.001 * np.random.default_rng(3).standard_normal(len(x))).astype(np.float32)
    for name, s in (("x.wav", x), ("y.wav", y), ("h.wav", h)):
        save_wav(str(tmp_path / name), torch.from_numpy(s), SR)
    lst = tmp_path / "t.txt"
    lst.write_text(" ---> ".join(str(tmp_path / n) for n in ("x.wav", "y.wav", "h.wav")) + "\n")
    res, out = run_cli(tmp_path, lst, "lra.csv", ["--loudness-range"], eval_cli.HOST_SCORER)
    capsys.readouterr()
    _, rows = read_csv(out)
    assert rows[0][8:] == [eval_cli.fmt(ld.loudness_range(s)) for s in (h, x, y)] and all(c == 1 for _, _, c in res.loudness_range)
    assert abs(float(rows[0][8]) - float(rows[0][9])) < 1e-6 and float(rows[0][9]) > 1.0      # a gain moves no range


def test_without_the_switches_every_byte_is_what_it_was(tmp_path, capsys):
    from flowdec_amd import eval_cli
    lst, _ = loudness_triples(tmp_path)

    def boom(*a, **k):
        raise AssertionError("a new measure was reached without its switch")

    H = eval_cli.HOST_SCORER
    old = eval_cli.Scorer(H.si_sxr, H.logspec, H.estoi, H.spectral, H.align, H.align_frac, H.shift, H.loudness, H.segsnr)      # the fields of before
    trap = eval_cli.Scorer(H.si_sxr, H.logspec, H.estoi, H.spectral, H.align, H.align_frac, H.shift, H.loudness, H.segsnr, boom, boom)
    assert old.loudness_range is None and old.true_peak is None and H.true_peak is not None and H.loudness_range is not None
    assert eval_cli.GPU_SCORER.true_peak is not None and eval_cli.GPU_SCORER.loudness_range is not None
    for flags in ([], ["--estoi", "--align", "1", "--align-polarity", "--loudness"], ["--match-loudness", "--ssnr"]):
        outs = []
        for name, scorer in (("a.csv", H), ("b.csv", old), ("c.csv", trap)):
            run_cli(tmp_path, lst, name, flags, scorer)
            outs.append(capsys.readouterr().out.replace(name, "x.csv"))
        assert (tmp_path / "a.csv").read_bytes() == (tmp_path / "b.csv").read_bytes() == (tmp_path / "c.csv").read_bytes()
        assert outs[0] == outs[1] == outs[2] and "lra_" not in outs[0] and "dbtp_" not in outs[0]
        header = (tmp_path / "a.csv").read_text().splitlines()[0]
        assert "lra_" not in header and "dbtp_" not in header
    # fixed expectations of the plain run: the header and the summary block it has always had
    run_cli(tmp_path, lst, "a.csv", [], H)
    plain = capsys.readouterr().out.splitlines()
    assert (tmp_path / "a.csv").read_text().splitlines()[0] == "name,x_hat,x,y,sisdr,sisir,sisar,logspec_mse"
    assert len(plain) == 5 and plain[0].startswith("eval: 6 triples, 6 rows in ") and [l.split()[0] for l in plain[1:]] == list(eval_cli.METRIC_NAMES)
    for flag in ("--loudness-range", "--true-peak"):
        with pytest.raises(AssertionError):
            run_cli(tmp_path, lst, "d.csv", [flag], trap)
        with pytest.raises(ValueError):
            run_cli(tmp_path, lst, "d.csv", [flag], old)
        capsys.readouterr()
        with pytest.raises(SystemExit):                       # a rate the measure does not take is a parser error before any file is read
            run_cli(tmp_path, tmp_path / "no_such_list.txt", "d.csv", [flag, "--sr", "47999"], H)
        assert "cap" in capsys.readouterr().err


def test_scorer_counts_the_new_functions_in_equality_hash_and_repr():
    import dataclasses
    from flowdec_amd import eval_cli
    H = eval_cli.HOST_SCORER
    f, g = (lambda *a: None), (lambda *a: None)
    base = (H.si_sxr, H.logspec, H.estoi, H.spectral, H.align, H.align_frac, H.shift, H.loudness, H.segsnr)
    a, b, c, d = eval_cli.Scorer(*base, f, g), eval_cli.Scorer(*base, f, g), eval_cli.Scorer(*base, g, g), eval_cli.Scorer(*base)
    assert a == b and hash(a) == hash(b) and a != c and a != d and c != d and d == eval_cli.Scorer(*base) and a != "x"
    assert len({a, b, c, d}) == 3 and "loudness_range=" in repr(a) and "true_peak=None" in repr(d)
    assert [x.name for x in dataclasses.fields(eval_cli.Scorer)][-1] == "segsnr" and eval_cli.Scorer(true_peak=f, si_sxr=f, logspec=g).true_peak is f
    with pytest.raises(dataclasses.FrozenInstanceError):
        a.true_peak = g
    r = a.replace(segsnr=None)                                # Scorer.replace carries the two functions over
    assert r.segsnr is None and r.loudness_range is f and r.true_peak is g and r.si_sxr is a.si_sxr and r != a
    assert a.replace(true_peak=None).true_peak is None and a.replace() == a
    with pytest.raises(TypeError):
        a.replace(no_such_function=f)


# ---- enhance_cli ---------------------------------------------------------------------------------------------------------------------------
class StubModel:
    """The surface enhance_cli.run uses, on the host: every output is the input at half the level (a pure function of the file)."""
    sampling_rate = SR
    device = "cpu"
    feature_extractor = types.SimpleNamespace(_cfg=lambda: {"hop": 384, "n_fft": 1534})

    def enhance(self, y, **kw):
        return y * 0.5

    def enhance_batch(self, clips, **kw):
        return [c * 0.5 for c in clips]


@pytest.fixture()
def corpus(tmp_path):
    """Five inputs: three mono tones of different levels and lengths (two of them share a T_pad bucket), a stereo file, and one under
    400 ms.  -> (input dir, {name: float32 [C, L]})."""
    import torch
    from flowdec_amd.audio import save_wav
    (tmp_path / "in").mkdir()
    rng = np.random.default_rng(12)
    files = {"a.wav": tone(1000.0, [(-20, 0.5)])[None], "b.wav": tone(440.0, [(-30, 0.45), (-24, 0.2)])[None], "c.wav": tone(3000.0, [(-12, 1.3)])[None],
             "d.wav": np.stack([tone(1000.0, [(-20, 0.6)]), tone(1000.0, [(-26, 0.6)])]), "e.wav": (0.1 * rng.standard_normal(6000)).astype(np.float32)[None]}
    for name, w in files.items():
        save_wav(str(tmp_path / "in" / name), torch.from_numpy(w), SR)
    return tmp_path / "in", files


def run_enhance(tmp_path, indir, out, *extra):
    from flowdec_amd import enhance_cli
    argv = ["--ckpt", "none.ckpt", "--files", str(indir), "--outdir", str(tmp_path / out), "--N", "1", "--batch-files", "2", *extra]
    return enhance_cli.run(argv, model=StubModel())


def host_level(monkeypatch, ld):
    """The level of a file from the host yardsticks instead of the GPU batch (the same bits: tests/test_hip_loudness_range.py)."""
    from flowdec_amd import enhance_cli
    seen = []

    def level(w, sr, args, peak=True):
        seen.append((tuple(w.shape), peak))
        lufs, dbtp = ld.file_level([c.numpy() for c in w.reshape(-1, w.shape[-1])], sr)
        return float(lufs), float(dbtp) if peak else float("nan")
    monkeypatch.setattr(enhance_cli, "_file_level", level)
    return seen


def read_level_csv(path):
    lines = path.read_text().splitlines()
    assert lines[0] == "name,lufs,dbtp,gain_db,limited"
    return {l.split(",")[0]: l.split(",")[1:] for l in lines[1:]}, [l.split(",")[0] for l in lines[1:]]


def test_enhance_cli_target_lufs(ld, tmp_path, corpus, monkeypatch, capsys):
    from flowdec_amd import enhance_cli
    from flowdec_amd.audio import load_wav
    indir, files = corpus
    seen = host_level(monkeypatch, ld)
    res = run_enhance(tmp_path, indir, "t23", "--target-lufs", "-23")
    assert len(seen) == 5 and all(peak for _, peak in seen)          # one measurement per written file
    err = capsys.readouterr().err
    assert res.n_done == 5 and sorted(os.listdir(tmp_path / "t23")) == sorted(list(files) + ["loudness.csv"])
    rows, order = read_level_csv(tmp_path / "t23" / "loudness.csv")
    assert sorted(order) == sorted(files) and len(order) == 5
    for name, w in files.items():
        half = [c * np.float32(0.5) for c in w]
        lufs, dbtp = ld.file_level(half)
        out = load_wav(str(tmp_path / "t23" / name))[0].numpy()
        if name == "e.wav":                                   # under 400 ms: no loudness, written as the model gave it, with a warning
            assert rows[name] == ["nan", enhance_cli.eval_cli.fmt(dbtp), "nan", "0"] and np.array_equal(out, np.stack(half))
            assert err.count("no level to set") == 1 and "e.wav" in err
            continue
        gain, limited = ld.output_gain(lufs, dbtp, -23.0, -1.0)
        assert rows[name] == [enhance_cli.eval_cli.fmt(lufs), enhance_cli.eval_cli.fmt(dbtp), enhance_cli.eval_cli.fmt(gain), "0"] and not limited
        assert np.array_equal(out, np.stack(half) * np.float32(10.0 ** (gain / 20.0)))             # ONE float32 multiply per sample
        # the written file re-measures at the target: 2^-24 relative on the samples and on the factor is under 1.1e-6 dB
        again = ld.file_level(list(out))[0]
        print(name, "re-measures at", again, "LUFS after", gain, "dB")
        assert abs(again - -23.0) <= 1e-4
    # --target-lufs input: every file comes back to the loudness of its own input (the model halved it: +6.02 dB)
    run_enhance(tmp_path, indir, "tin", "--target-lufs", "input", "--peak-ceiling", "0")
    capsys.readouterr()
    rows, _ = read_level_csv(tmp_path / "tin" / "loudness.csv")
    assert len(seen) == 15 and sum(1 for _, peak in seen[5:] if not peak) == 5      # the input's loudness is taken without its true peak
    for name, w in files.items():
        if name == "e.wav":
            continue
        out = load_wav(str(tmp_path / "tin" / name))[0].numpy()
        assert abs(ld.file_level(list(out))[0] - ld.file_level(list(w))[0]) <= 1e-4 and abs(float(rows[name][2]) - 20 * math.log10(2.0)) <= 1e-6
    with pytest.raises(SystemExit):
        enhance_cli.build_parser().parse_args(["--ckpt", "c", "--files", "f", "--outdir", "o", "--N", "1", "--target-lufs", "loud"])
    assert "finite number of LUFS" in capsys.readouterr().err


def test_enhance_cli_peak_ceiling(ld, tmp_path, corpus, monkeypatch, capsys):
    from flowdec_amd import enhance_cli
    from flowdec_amd.audio import load_wav
    indir, files = corpus
    host_level(monkeypatch, ld)
    # a target far above the files: the ceiling caps every gain, and the written peaks land on it
    run_enhance(tmp_path, indir, "cap", "--target-lufs", "0", "--peak-ceiling", "-2.5")
    rows, _ = read_level_csv(tmp_path / "cap" / "loudness.csv")
    for name, w in files.items():
        if name == "e.wav":
            continue
        lufs, dbtp = ld.file_level([c * np.float32(0.5) for c in w])
        assert rows[name] == [enhance_cli.eval_cli.fmt(lufs), enhance_cli.eval_cli.fmt(dbtp), enhance_cli.eval_cli.fmt(-2.5 - dbtp), "1"]
        out = load_wav(str(tmp_path / "cap" / name))[0].numpy()
        assert abs(ld.file_level(list(out))[1] - -2.5) <= 1e-4 and ld.file_level(list(out))[0] < 0.0
    # --peak-ceiling alone: 0 dB for the files under it (their bytes are the plain run's), the others turned down to it
    run_enhance(tmp_path, indir, "plain")
    run_enhance(tmp_path, indir, "ceil", "--peak-ceiling", "-20")
    capsys.readouterr()
    rows, _ = read_level_csv(tmp_path / "ceil" / "loudness.csv")
    over = 0
    for name, w in files.items():
        dbtp = ld.file_level([c * np.float32(0.5) for c in w])[1]
        a, b = (tmp_path / "plain" / name).read_bytes(), (tmp_path / "ceil" / name).read_bytes()
        if dbtp > -20.0:
            over += 1
            assert rows[name][2:] == [enhance_cli.eval_cli.fmt(-20.0 - dbtp), "1"] and a != b
            assert abs(ld.file_level(list(load_wav(str(tmp_path / "ceil" / name))[0].numpy()))[1] - -20.0) <= 1e-4
        else:
            assert rows[name][2:] == ["0.0", "0"] and a == b
    assert 1 <= over <= 4 and rows["e.wav"][0] == "nan"          # the short file has a peak, so the ceiling holds for it too


def test_enhance_cli_without_the_switches_nothing_changes(ld, tmp_path, corpus, monkeypatch, capsys):
    import torch
    from flowdec_amd import enhance_cli
    from flowdec_amd.audio import save_wav
    indir, files = corpus
    monkeypatch.setattr(enhance_cli, "_file_level", lambda *a: pytest.fail("the level was measured without its switches"))
    res = run_enhance(tmp_path, indir, "plain")
    out = capsys.readouterr()
    assert res.n_done == 5 and sorted(os.listdir(tmp_path / "plain")) == sorted(files) and "warning" not in out.err
    for name, w in files.items():                             # fixed expectations: the stub's output, saved as it always was
        save_wav(str(tmp_path / "want.wav"), torch.from_numpy(w) * 0.5, SR)
        assert (tmp_path / "plain" / name).read_bytes() == (tmp_path / "want.wav").read_bytes()
    args = enhance_cli.build_parser().parse_args(["--ckpt", "c", "--files", "f", "--outdir", "o", "--N", "1"])
    assert args.target_lufs is None and args.peak_ceiling is None and not enhance_cli.level_wanted(args)
    assert not args.eval_loudness_range and not args.eval_true_peak
    args = enhance_cli.build_parser().parse_args(["--ckpt", "c", "--files", "f", "--outdir", "o", "--N", "1", "--target-lufs", "INPUT"])
    assert args.target_lufs == "input" and args.peak_ceiling is None and enhance_cli.level_wanted(args)


def test_enhance_cli_merges_the_level_parts_and_passes_the_switches_on(tmp_path, monkeypatch):
    import argparse
    import contextlib
    import json
    import torch
    from flowdec_amd import enhance_cli, eval_cli
    from flowdec_amd.enhance_cli import FileJob, level_part_name, merge_parts, result_part_name
    parts = {0: ["2,c.wav,-30.5,-12.0,7.5,0", "0,a.wav,-20.0,-3.0,2.0,1", "0,b.wav,nan,-40.0,nan,0"], 1: ["1,d.wav,-inf,-inf,nan,0"]}
    for r in range(2):
        (tmp_path / level_part_name("", r)).write_text("\n".join(["position,name,lufs,dbtp,gain_db,limited"] + parts[r]) + "\n")
        (tmp_path / result_part_name("", r)).write_text(json.dumps(dict(n_done=len(parts[r]), n_over_precision_limit=0, n_too_long=0, gpu_seconds=0.0,
                                                                         audio_seconds=0.0)))
    res = merge_parts(str(tmp_path), "", 2, [FileJob(0, "a", "b", None, True)], want_rtf=False, want_triples=False, want_level=True)
    assert res.n_done == 4 and sorted(os.listdir(tmp_path)) == ["loudness.csv"]
    assert (tmp_path / "loudness.csv").read_text() == ("name,lufs,dbtp,gain_db,limited\na.wav,-20.0,-3.0,2.0,1\nb.wav,nan,-40.0,nan,0\nd.wav,-inf,-inf,nan,0\n"
                                                        "c.wav,-30.5,-12.0,7.5,0\n")
    seen = []
    monkeypatch.setattr(eval_cli, "run", lambda argv, **k: seen.append(list(argv)))
    monkeypatch.setattr(torch.cuda, "device", lambda d: contextlib.nullcontext())
    ns = argparse.Namespace(outdir="o", batch_files=4, device=0, eval_loudness=True, eval_loudness_range=True, eval_true_peak=True, eval_ssnr=True)
    enhance_cli.evaluate_triples(ns, "")
    assert seen[0][-4:] == ["--loudness", "--loudness-range", "--true-peak", "--ssnr"]
    ns.eval_loudness_range = ns.eval_true_peak = False
    enhance_cli.evaluate_triples(ns, "")
    assert seen[1][-2:] == ["--loudness", "--ssnr"]


# ---- the library ---------------------------------------------------------------------------------------------------------------------------
def test_symbols_in_the_header_the_table_and_the_build(ld):
    import __graft_entry__ as g
    g.build()
    from flowdec_amd import _lib
    lib = _lib.load()
    src = open(os.path.join(g.ROOT, "include", "flowdec_hip.h")).read()
    for name in ("fd_true_peak_tile", "fd_true_peak_workspace_bytes", "fd_true_peak", "fd_loudness_range_workspace_bytes", "fd_loudness_range"):
        assert name + "(" in src and hasattr(lib, name) and name in _lib.SIGNATURES
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
    assert "loudness_range.hip" in __import__("flowdec_amd.build", fromlist=["SOURCES"]).SOURCES
    T = lib.fd_true_peak_tile()
    assert T >= 64 and T % 64 == 0
    # refusals need no GPU: every call below refuses before a launch
    err = lambda: lib.fd_last_error().decode()                       # noqa: E731
    p = C.c_void_p(64)
    need = lib.fd_true_peak_workspace_bytes(2, 48000)
    assert need > 0 and lib.fd_true_peak_workspace_bytes(1, 1) > 0 and lib.fd_true_peak_workspace_bytes(2, 10 * 48000) > need
    for B, Lr in ((0, 48000), (-1, 48000), (65536, 48000), (2, 0), (2, -5)):
        assert lib.fd_true_peak_workspace_bytes(B, Lr) == 0
    peak = lambda x=p, lens=p, B=2, Lr=48000, lo=p, hi=p, taps=p, W=12, out=p, ws=p, n=1 << 40: lib.fd_true_peak(x, lens, B, Lr, lo, hi, taps, W, out, ws, n, None)   # noqa: E731
    for kw, word in (({"x": None}, "null"), ({"lens": None}, "null"), ({"out": None}, "null"), ({"taps": None}, "taps"), ({"ws": None}, "ws"),
                     ({"lo": None}, "both"), ({"hi": None}, "both"), ({"B": 0}, "batch"), ({"B": 65536}, "batch"), ({"Lr": 0}, "row length"),
                     ({"W": 0}, "half width"), ({"W": 257}, "half width")):
        assert peak(**kw) == FD_EINVAL and word in err(), kw
    assert peak(n=need - 1) == FD_ENOMEM and "workspace too small" in err()
    need = lib.fd_loudness_range_workspace_bytes(2, 700)
    assert need > 0 and lib.fd_loudness_range_workspace_bytes(1, 0) > 0 and lib.fd_loudness_range_workspace_bytes(2, 36030) > need
    for B, J in ((0, 700), (65536, 700), (2, -1), (2, 1 << 30)):
        assert lib.fd_loudness_range_workspace_bytes(B, J) == 0
    rng_ = lambda E=p, nsub=p, B=2, J=700, st=p, counts=p, ws=p, n=1 << 40: lib.fd_loudness_range(E, nsub, B, J, st, counts, ws, n, None)   # noqa: E731
    for kw, word in (({"E": None}, "E"), ({"nsub": None}, "null"), ({"st": None}, "null"), ({"counts": None}, "null"), ({"ws": None}, "ws"),
                     ({"B": 0}, "batch"), ({"J": -1}, "Jmax"), ({"J": 1 << 30}, "Jmax")):
        assert rng_(**kw) == FD_EINVAL and word in err(), kw
    assert rng_(n=need - 1) == FD_ENOMEM and "workspace too small" in err()
