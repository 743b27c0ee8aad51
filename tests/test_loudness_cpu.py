"""flowdec_amd/loudness.py on the host: the yardstick of csrc/loudness.hip against the conformance readings of ITU-R BS.1770-4 and EBU Tech
3341 (in mono), against an independent scipy.signal.lfilter reading, its defining properties, match_loudness, and eval_cli --loudness /
--match-loudness on the host scorer.  No GPU."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

from loudness_cases import (QUIET_DB, REF_BOUND_DB, REF_MAX_OBSERVED_DB, SHORT, SR, loudness_triples, reference_inputs, reference_reading, tone)
from test_align_cpu import FD_EINVAL, FD_ENOMEM
from test_eval_cpu import read_csv

# one float32 multiply per sample moves every sample by at most 2^-24 relative, the energy of any stretch by at most 2 * 2^-24 (and
# 2^-48), so the loudness by 10 log10(1 + 2^-23) dB; the factor itself is rounded to float32 once: another 2^-24 on every sample alike
ONE_MULTIPLY_DB = 10 * math.log10(1 + 2.0 ** -23 + 2.0 ** -48)
MATCH_BOUND_DB = 2 * ONE_MULTIPLY_DB + 1e-12


@pytest.fixture(scope="module")
def ld():
    from flowdec_amd import loudness
    return loudness


@pytest.fixture(scope="module")
def ref_inputs(ld):
    return reference_inputs(ld.K48, ld.ABS_GATE)


def test_tables_and_constants(ld):
    assert ld.K48[0] == (1.53512485958697, -2.69169618940638, 1.19839281085285, -1.69065929318241, 0.73248077421585)
    assert ld.K48[1] == (1.0, -2.0, 1.0, -1.99004745483398, 0.99007225036621)
    assert ld.ABS_GATE == 10.0 ** ((-70 + 0.691) / 10) == 1.1724653045822981e-07 and ld.SUB % ld.CHUNK == 0 and ld.NCHUNK == 64
    # the transition matrices are what the step does to a state with no input: 75 steps 64 times over is 4800 steps, up to rounding
    # (the high-pass has a pole pair close to z = 1, so the power loses digits: 4e-8 relative was seen)
    P = np.linalg.matrix_power(ld.M_CHUNK, 64)
    assert np.max(np.abs(P - ld.M_SUB)) <= 1e-6 * np.max(np.abs(ld.M_SUB))
    s = [np.float64(v) for v in (0.3, -0.2, 0.1, 0.05)]
    want = ld.M_CHUNK @ np.array(s)
    for _ in range(ld.CHUNK):
        ld._kstep(np.float64(0.0), s)
    assert np.allclose(np.array(s), want, rtol=1e-12, atol=1e-15)


@pytest.mark.parametrize("dbfs,want", [(0.0, -3.01), (-23.0, -26.01)])
def test_conformance_997_hz_sine(ld, dbfs, want):
    """BS.1770-4: a 0 dBFS 997 Hz sine in one front channel reads -3.01 LKFS; the bound is the standard's two decimals."""
    got = ld.integrated_loudness(tone(997.0, [(dbfs, 20.0)]))
    print("997 Hz at", dbfs, "dBFS reads", got)
    assert abs(got - want) <= 0.01


@pytest.mark.parametrize("steps", [[(-36, 10), (-23, 60), (-36, 10)], [(-72, 10), (-36, 10), (-23, 60), (-36, 10), (-72, 10)],
                                   [(-26, 20), (-20, 20.1), (-26, 20)]], ids=["relative-gate", "absolute-gate", "both"])
def test_conformance_tone_sequences(ld, steps):
    """EBU Tech 3341 cases 3, 4 and 5 in mono (one channel of the stereo signals that read -23.0 LUFS): -26.0 +- 0.1 LUFS."""
    x = tone(1000.0, steps)
    got = ld.integrated_loudness(x)
    ref = reference_reading(x, ld.K48, ld.ABS_GATE)[0]
    print(steps, "reads", got, "scipy", ref)
    assert abs(got - (-26.0)) <= 0.1 and abs(got - ref) <= 1e-9


def test_independent_reference(ld, ref_inputs):
    """scipy.signal.lfilter + literal block loops on seeded noise with a silent stretch and a quiet half.  Counts equal; LUFS within
    REF_BOUND_DB = 16 x the largest difference observed on these very inputs on the host (1.25e-14 dB -> 2e-13 dB; never taken from the
    kernel), which itself is far below 1e-9 dB."""
    worst = 0.0
    for x, want, want_counts in ref_inputs:
        E = ld.kweight_energies(x)
        ms, counts = ld.gate(E)
        got = ld.lufs_of(ms)
        assert E.shape == (len(x) // 4800,) and counts.tolist() == want_counts.tolist() and counts[2] >= 1
        worst = max(worst, abs(got - want))
        print(len(x), "samples:", got, "LUFS, counts", counts.tolist(), "difference", got - want)
        assert abs(got - want) <= REF_BOUND_DB
        assert got == ld.integrated_loudness(x)
    print("largest difference", worst, "dB; recorded", REF_MAX_OBSERVED_DB)
    assert REF_BOUND_DB == 16 * REF_MAX_OBSERVED_DB < 1e-9
    # the long input exercises both gates
    assert ref_inputs[-1][2][0] > ref_inputs[-1][2][1] > ref_inputs[-1][2][2]


def test_power_of_two_scaling_is_exact(ld, ref_inputs):
    x = ref_inputs[3][0]
    ms, counts = ld.gate(ld.kweight_energies(x))
    for k in (-3, 1, 4):
        ms_k, counts_k = ld.gate(ld.kweight_energies(x * np.float32(2.0 ** k)))
        assert ms_k == ms * 4.0 ** k and ms_k > 0
        # (the absolute gate does not scale: the input keeps every block clear of it by more than these factors)
        assert counts_k.tolist() == counts.tolist()


def test_tail_is_not_read_and_the_length_rules(ld, ref_inputs):
    x = ref_inputs[3][0].copy()                        # 100003 samples: 20 sub-blocks and a tail of 4003
    E = ld.kweight_energies(x)
    x[20 * 4800:] = np.nan
    assert np.array_equal(ld.kweight_energies(x), E) and math.isfinite(ld.integrated_loudness(x))
    x[20 * 4800 - 1] = np.nan
    assert math.isnan(ld.integrated_loudness(x))       # the last sample that is read
    ms, counts = ld.gate(ld.kweight_energies(x))
    assert math.isnan(ms) and counts.tolist() == [17, 0, 0]
    y = ref_inputs[0][0]
    ms, counts = ld.gate(ld.kweight_energies(y[:19199]))
    assert math.isnan(ms) and counts.tolist() == [0, 0, 0] and math.isnan(ld.integrated_loudness(y[:19199]))
    assert ld.gate(ld.kweight_energies(y))[1][0] == 1
    z = np.zeros(48000, np.float32)
    assert ld.integrated_loudness(z) == float("-inf") and ld.gate(ld.kweight_energies(z))[1].tolist() == [7, 0, 0]
    z[100] = np.inf
    assert math.isnan(ld.integrated_loudness(z))
    with pytest.raises(TypeError):
        ld.integrated_loudness(np.zeros(48000, np.float64))


def test_state_hand_over_and_windows(ld, ref_inputs):
    """Cut at any multiple of 4800 samples with the state handed on: the same bits (what LoudnessMeter rests on)."""
    x = ref_inputs[3][0]
    E = ld.kweight_energies(x)
    for cut in (4800, 9 * 4800):
        Ea, state = ld.kweight_energies(x[:cut], return_state=True)
        Eb = ld.kweight_energies(x[cut:], state=state)
        assert np.array_equal(np.concatenate([Ea, Eb]), E)
    assert ld.momentary_of(E) == ld.lufs_of((((E[-4] + E[-3]) + E[-2]) + E[-1]) / 19200.0)
    assert math.isnan(ld.short_term_of(E)) and math.isnan(ld.momentary_of(E[:3]))
    E30 = np.concatenate([E, E])[:30]
    assert abs(ld.short_term_of(E30) - ld.lufs_of(E30.sum() / 144000.0)) < 1e-12


def test_other_rates_resample_first(ld):
    from flowdec_amd import audio
    x = tone(997.0, [(-20.0, 2.0)], sr=16000)
    up = audio.resample(torch.from_numpy(x), 16000, 48000, lowpass_filter_width=64).numpy()
    assert ld.integrated_loudness(x, 16000) == ld.integrated_loudness(up)
    assert abs(ld.integrated_loudness(x, 16000) - (-23.01)) < 0.02
    with pytest.raises(ValueError, match="cap"):
        ld.integrated_loudness(x, 47999)
    with pytest.raises(ValueError, match="cap"):
        ld.check_rate(44101)


def test_match_loudness(ld, ref_inputs):
    """After matching, the re-measured loudness is the target within the rounding of one float32 multiply (MATCH_BOUND_DB, derived at
    the top of this file)."""
    x = ref_inputs[2][0]
    l0 = ld.integrated_loudness(x)
    for target in (-16.0, -23.0, l0 + 6.0, l0 - 2.5):
        g = ld.gain_factor(l0, target)
        assert g.dtype == np.float32 and g == np.float32(10.0 ** ((target - l0) / 20.0)) and ld.gain_db(l0, target) == target - l0
        y = ld.match_loudness(x, l0, target)
        assert y.dtype == np.float32 and np.array_equal(y, x * g)
        t = ld.match_loudness(torch.from_numpy(x), l0, target)
        assert t.dtype == torch.float32 and np.array_equal(t.numpy(), y)
        got = ld.integrated_loudness(y)
        print("target", target, "re-measured", got, "bound", MATCH_BOUND_DB)
        assert abs(got - target) <= MATCH_BOUND_DB
    with pytest.raises(ValueError):
        ld.match_loudness(x, float("-inf"), -23.0)


def run_cli(tmp_path, lst, name, flags, scorer):
    from flowdec_amd import eval_cli
    out = tmp_path / name
    res = eval_cli.run(["--triples", str(lst), "--out", str(out), "--batch-files", "2"] + flags, scorer=scorer)
    return res, out


def test_eval_cli_loudness_columns_and_matching(ld, tmp_path, capsys):
    from flowdec_amd import eval_cli, metrics
    lst, sigs = loudness_triples(tmp_path)
    H = eval_cli.HOST_SCORER
    base, out_base = run_cli(tmp_path, lst, "base.csv", [], H)
    capsys.readouterr()
    loud, out_loud = run_cli(tmp_path, lst, "loud.csv", ["--loudness"], H)
    cap_loud = capsys.readouterr()
    match, out_match = run_cli(tmp_path, lst, "match.csv", ["--match-loudness"], H)
    cap_match = capsys.readouterr()
    full, out_full = run_cli(tmp_path, lst, "full.csv", ["--estoi", "--align", "1", "--loudness"], H)
    capsys.readouterr()
    h0, r0 = read_csv(out_base)
    h1, r1 = read_csv(out_loud)
    h2, r2 = read_csv(out_match)
    h3, _ = read_csv(out_full)
    assert tuple(h1) == tuple(h2) == eval_cli.CSV_HEADER + ("lufs_x_hat", "lufs_x", "lufs_y") == eval_cli.CSV_HEADER + eval_cli.LUFS_NAMES
    assert tuple(h3) == eval_cli.CSV_HEADER + ("estoi", "lufs_x_hat", "lufs_x", "lufs_y", "lag_x_hat", "lag_y")
    # --loudness touches no other column; the three columns are the yardstick's reading of the signals, before matching in both runs
    assert [r[:8] for r in r1] == r0
    want = [[eval_cli.fmt(ld.integrated_loudness(s)) for s in t] for t in sigs]
    assert [r[8:] for r in r1] == want == [r[8:] for r in r2]
    assert r1[SHORT][8:] == ["nan", "nan", "nan"]
    for i, db in QUIET_DB.items():
        assert abs((float(r1[i][8]) - float(r1[i][9])) - db) < 0.05
    # the summary: three more lines
    assert [n for n, _, _ in loud.loudness] == list(eval_cli.LUFS_NAMES) and all(c == 5 for _, _, c in loud.loudness) and base.loudness == []
    assert "lufs_x_hat   mean = " in cap_loud.out and "over 5 finite rows" in cap_loud.out
    # --match-loudness: the quiet rows score as the same files scaled by hand with the yardstick's factor
    for i, (h, x, y) in enumerate(sigs):
        if i == SHORT:
            assert r2[i][:8] == r0[i]                         # left unscaled
            continue
        lh, lx = ld.integrated_loudness(h), ld.integrated_loudness(x)
        by_hand = metrics.logspec_mse(h * np.float32(10.0 ** ((lx - lh) / 20.0)), x, sr=SR, win_dur=eval_cli.WIN_DUR, hop_dur=eval_cli.HOP_DUR)
        got, before = float(r2[i][7]), float(r0[i][7])
        print("triple", i, "logspec_mse", before, "->", got, "by hand", by_hand)
        # (the same float32 samples through the same function: the one-multiply bound of 2^-23 on a power is 4.4e-7 dB per bin)
        assert abs(got - by_hand) <= 1e-6 * max(1.0, by_hand)
        if i in QUIET_DB:
            assert got < 0.2 * before
        assert abs(float(r2[i][4]) - float(r0[i][4])) < 1e-2     # SI-SDR is scale-invariant (the host function sums in float32)
    warned = [l for l in cap_match.err.splitlines() if "no loudness to match" in l]
    assert len(warned) == 2 and all(f"enh_{SHORT}.wav" in l for l in warned) and "no loudness to match" not in cap_loud.err
    assert match.exit_code == 0 and match.n_scored == 6


def test_without_the_switches_every_byte_is_what_it_was(tmp_path, capsys):
    from flowdec_amd import eval_cli
    lst, _ = loudness_triples(tmp_path)

    def boom(*a, **k):
        raise AssertionError("the loudness path was reached without its switches")

    H = eval_cli.HOST_SCORER
    old = eval_cli.Scorer(H.si_sxr, H.logspec, H.estoi, H.spectral, H.align, H.align_frac, H.shift)      # the fields of before
    trap = eval_cli.Scorer(H.si_sxr, H.logspec, H.estoi, H.spectral, H.align, H.align_frac, H.shift, boom)
    assert old.loudness is None and H.loudness is not None and eval_cli.GPU_SCORER.loudness is not None
    for flags in ([], ["--estoi", "--align", "1", "--align-polarity"]):
        outs = []
        for name, scorer in (("a.csv", H), ("b.csv", old), ("c.csv", trap)):
            run_cli(tmp_path, lst, name, flags, scorer)
            outs.append(capsys.readouterr().out.replace(name, "x.csv"))
        assert (tmp_path / "a.csv").read_bytes() == (tmp_path / "b.csv").read_bytes() == (tmp_path / "c.csv").read_bytes()
        assert outs[0] == outs[1] == outs[2] and "lufs" not in outs[0]
    with pytest.raises(AssertionError):
        run_cli(tmp_path, lst, "d.csv", ["--loudness"], trap)
    with pytest.raises(ValueError):
        run_cli(tmp_path, lst, "d.csv", ["--match-loudness"], old)
    with pytest.raises(ValueError, match="cap"):          # a rate the resampler in front of the measure does not take
        eval_cli.measure_loudness([], 47999, 2, H)
    capsys.readouterr()
    with pytest.raises(SystemExit):                       # ... is a parser error before any file is read
        run_cli(tmp_path, tmp_path / "no_such_list.txt", "d.csv", ["--loudness", "--sr", "47999"], H)
    assert "cap" in capsys.readouterr().err


def test_enhance_cli_passes_the_switches_on(monkeypatch):
    import argparse
    import contextlib
    from flowdec_amd import enhance_cli, eval_cli
    seen = []
    monkeypatch.setattr(eval_cli, "run", lambda argv, **k: seen.append(list(argv)))
    monkeypatch.setattr(torch.cuda, "device", lambda d: contextlib.nullcontext())
    ns = argparse.Namespace(outdir="o", batch_files=4, device=0, eval_estoi=False, eval_spectral=False, eval_align=None, eval_align_frac=False,
                            eval_align_polarity=False, eval_loudness=True, eval_match_loudness=True)
    enhance_cli.evaluate_triples(ns, "")
    assert seen and seen[0][-2:] == ["--loudness", "--match-loudness"]
    ns.eval_match_loudness = False
    enhance_cli.evaluate_triples(ns, "")
    assert seen[1][-1] == "--loudness"
    ns.eval_loudness = False
    enhance_cli.evaluate_triples(ns, "")
    assert "--loudness" not in seen[2] and "--match-loudness" not in seen[2]
    assert {"eval_loudness", "eval_match_loudness"} <= {a.dest for a in enhance_cli.build_parser()._actions}
    args = eval_cli.build_parser().parse_args(["--triples", "t", "--out", "o", "--match-loudness"])
    assert args.match_loudness and not args.loudness


def test_symbols_in_the_header_the_table_and_the_build(ld):
    import __graft_entry__ as g
    g.build()
    from flowdec_amd import _lib
    lib = _lib.load()
    src = open(os.path.join(g.ROOT, "include", "flowdec_hip.h")).read()
    for name in ("fd_loudness_tables", "fd_loudness_workspace_bytes", "fd_loudness_energies", "fd_loudness_gate", "fd_loudness"):
        assert name + "(" in src and hasattr(lib, name) and name in _lib.SIGNATURES
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
    assert "loudness.hip" in __import__("flowdec_amd.build", fromlist=["SOURCES"]).SOURCES
    # the library's tables are the module's, bit for bit (built on the host by the same steps in the same order)
    mc, ms, gate = ld.device_tables()
    assert np.array_equal(mc, ld.M_CHUNK) and np.array_equal(ms, ld.M_SUB) and gate == ld.ABS_GATE
    # refusals need no GPU: every call below refuses before a launch
    err = lambda: lib.fd_last_error().decode()
    p = C.c_void_p(64)
    need = lib.fd_loudness_workspace_bytes(2, 48000)
    assert need > 0 and lib.fd_loudness_workspace_bytes(2, 100) > 0 and lib.fd_loudness_workspace_bytes(1, 4800) < need
    for B, Lr in ((0, 48000), (-1, 48000), (65536, 48000), (2, 0), (2, -5)):
        assert lib.fd_loudness_workspace_bytes(B, Lr) == 0
    one = lambda x=p, lens=p, B=2, Lr=48000, ms=p, counts=p, ws=p, n=1 << 40: lib.fd_loudness(x, lens, B, Lr, ms, counts, ws, n, None)
    for kw in (dict(x=None), dict(lens=None), dict(ms=None), dict(counts=None), dict(ws=None)):
        assert one(**kw) == FD_EINVAL and "fd_loudness:" in err() and "null pointer" in err(), (kw, err())
    for kw, word in ((dict(B=0), "B 0"), (dict(B=-2), "B -2"), (dict(Lr=0), "L 0"), (dict(ws=C.c_void_p(68)), "aligned")):
        assert one(**kw) == FD_EINVAL and "fd_loudness:" in err() and word in err(), (kw, err())
    assert one(n=need - 1) == FD_ENOMEM and "workspace" in err() and one(n=0) == FD_ENOMEM
    en = lambda x=p, lens=p, B=2, Lr=48000, state=None, E=p, nsub=p, ws=p, n=1 << 40: lib.fd_loudness_energies(x, lens, B, Lr, state, E, nsub, ws, n, None)
    for kw in (dict(x=None), dict(lens=None), dict(E=None), dict(nsub=None), dict(ws=None)):
        assert en(**kw) == FD_EINVAL and "fd_loudness_energies" in err() and "null pointer" in err(), (kw, err())
    for kw, word in ((dict(B=0), "B 0"), (dict(Lr=0), "L 0")):
        assert en(**kw) == FD_EINVAL and "fd_loudness_energies" in err() and word in err(), (kw, err())
    assert en(n=need - 1) == FD_ENOMEM and "workspace" in err()
    ga = lambda E=p, nsub=p, B=2, J=10, ms=p, counts=p: lib.fd_loudness_gate(E, nsub, B, J, ms, counts, None)
    for kw in (dict(E=None), dict(nsub=None), dict(ms=None), dict(counts=None)):
        assert ga(**kw) == FD_EINVAL and "fd_loudness_gate" in err() and "null pointer" in err(), (kw, err())
    for kw, word in ((dict(B=0), "B 0"), (dict(J=-1), "Jmax -1")):
        assert ga(**kw) == FD_EINVAL and "fd_loudness_gate" in err() and word in err(), (kw, err())
    assert lib.fd_loudness_tables(None, p, p) == FD_EINVAL and "fd_loudness_tables" in err()
