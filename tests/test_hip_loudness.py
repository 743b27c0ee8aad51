"""csrc/loudness.hip against its yardstick flowdec_amd/loudness.py, bit for bit: the K-weighted sub-block energies and the gated mean square
of ragged batches, batch invariance, exact power-of-two scaling, the streaming meter, other rates, the edge cases, the refusals, and
eval_cli --loudness / --match-loudness on the GPU scorer."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from loudness_cases import REF_BOUND_DB, SHORT, enveloped_noise, loudness_triples
from test_align_cpu import FD_EINVAL, FD_ENOMEM
from test_eval_cpu import read_csv

pytestmark = pytest.mark.gpu

CH = 75                      # the kernel's chunk: one lane
# around the chunk, the sub-block and the block edges
LENGTHS = (1, CH - 1, CH, CH + 1, 3 * CH + 5, 4799, 4800, 4801, 19199, 19200, 24000, 48000, 100003)


def same_bits(a, b):
    a, b = np.asarray(a, np.float64).reshape(-1), np.asarray(b, np.float64).reshape(-1)
    if a.shape != b.shape or not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    ok = ~np.isnan(a)
    return np.array_equal(a[ok].view(np.uint64), b[ok].view(np.uint64))


@pytest.fixture(scope="module")
def ld():
    from flowdec_amd import loudness
    return loudness


@pytest.fixture(scope="module")
def clips():
    """One seeded clip per LENGTHS entry, then a 0.2 s burst followed by 4 s of digital zeros (the filter state decays through the
    float64 subnormals there)."""
    out = [enveloped_noise(n, 500 + k) for k, n in enumerate(LENGTHS)]
    burst = np.zeros(9600 + 4 * 48000, np.float32)
    burst[:9600] = (0.5 * np.random.default_rng(77).standard_normal(9600)).astype(np.float32)
    return out + [burst]


@pytest.fixture(scope="module")
def yard(ld, clips):
    """The yardstick's (E, ms_gated, counts) of every clip, computed once."""
    out = []
    for x in clips:
        E = ld.kweight_energies(x)
        out.append((E,) + ld.gate(E))
    return out


def raw_rows(clips, Lrow, fill=float("nan")):
    """Rows [B, Lrow] on the device with `fill` behind every clip's end, and the int32 lengths."""
    rows = torch.full((len(clips), Lrow), fill, dtype=torch.float32)
    for b, c in enumerate(clips):
        rows[b, :len(c)] = torch.from_numpy(np.ascontiguousarray(c))
    return rows.cuda(), torch.tensor([len(c) for c in clips], dtype=torch.int32).cuda()


def raw_loudness(rows, lens):
    from flowdec_amd import _lib as L
    lib = L.load()
    B, Lrow = rows.shape
    nws = lib.fd_loudness_workspace_bytes(B, Lrow)
    assert nws > 0
    ws = torch.empty(nws, dtype=torch.uint8, device="cuda")
    ms = torch.empty(B, dtype=torch.float64, device="cuda")
    counts = torch.empty(B, 3, dtype=torch.int32, device="cuda")
    L.check(lib.fd_loudness(L.ptr(rows), L.ptr(lens), B, Lrow, L.ptr(ms), L.ptr(counts), L.ptr(ws), nws, L.stream()))
    return ms.cpu().numpy(), counts.cpu().numpy()


def test_energies_and_loudness_equal_the_yardstick_bit_for_bit(ld, clips, yard):
    E = ld.energies_batch(clips, batch=4)
    ms, counts = ld.loudness_ms_batch(clips, batch=4)
    for k, (x, (E_want, ms_want, counts_want)) in enumerate(zip(clips, yard)):
        assert E[k].shape == (len(x) // 4800,) and same_bits(E[k], E_want), f"clip {k} ({len(x)} samples): energies differ"
        assert same_bits(ms[k], ms_want) and counts[k].tolist() == counts_want.tolist(), f"clip {k} ({len(x)} samples): {ms[k]!r} vs {ms_want!r}"
    # the burst: its late sub-blocks are subnormal or zero energies, and still the same bits
    assert E[-1][0] > 1.0 and 0.0 < E[-1][17] < E[-1][16] < 1e-290 and E[-1][-1] == 0.0 and math.isfinite(ms[-1]) and counts[-1].tolist() == [39, 3, 2]
    assert np.array_equal(np.isnan(ms), np.array([len(x) < 19200 for x in clips]))
    lufs = ld.loudness_batch(clips, batch=4)
    assert same_bits(lufs, ld.lufs_of(np.array([m for _, m, _ in yard])))


def test_a_clip_has_the_same_bits_alone_and_anywhere_in_a_ragged_batch(ld, clips, yard):
    k = LENGTHS.index(100003)
    x = clips[k]
    alone = raw_loudness(*raw_rows([x], len(x)))
    assert same_bits(alone[0][0], yard[k][1]) and alone[1][0].tolist() == yard[k][2].tolist()
    others = [clips[LENGTHS.index(n)] for n in (24000, 4801, 48000, 19199)]
    for pos in (0, 2, 4):
        batch = others[:pos] + [x] + others[pos:]
        ms, counts = raw_loudness(*raw_rows(batch[:5], 100003 + 77))            # NaN behind every clip's end, a row longer than any clip
        assert same_bits(ms[pos], alone[0][0]) and counts[pos].tolist() == alone[1][0].tolist(), pos
    ms2, counts2 = ld.loudness_ms_batch(clips, batch=2)
    ms4, counts4 = ld.loudness_ms_batch(clips, batch=len(clips))
    assert same_bits(ms2, ms4) and np.array_equal(counts2, counts4) and same_bits(ms2[k], alone[0][0])
    # a lengths entry beyond L is clamped to L
    rows, lens = raw_rows([x, clips[LENGTHS.index(48000)]], len(x), fill=0.0)
    lens[0] = len(x) + 5000
    ms, counts = raw_loudness(rows, lens)
    assert same_bits(ms[0], alone[0][0]) and counts[0].tolist() == alone[1][0].tolist()


def test_power_of_two_scaling_is_exact(ld, clips, yard):
    k = LENGTHS.index(100003)
    for e in (-3, 1, 4):
        ms, counts = ld.loudness_ms_batch([clips[k] * np.float32(2.0 ** e)])
        assert ms[0] == yard[k][1] * 4.0 ** e and counts[0].tolist() == yard[k][2].tolist()


def feed(meter, x, sizes):
    """x cut into pushes of the sizes of `sizes`, cycled."""
    i = k = 0
    while i < len(x):
        n = sizes[k % len(sizes)]
        meter.push(x[i:i + n])
        i, k = i + n, k + 1
    return meter


def test_streaming_meter_equals_the_one_shot_call(ld):
    x = enveloped_noise(110400, 900)                   # 2.3 s: 23 sub-blocks
    q = np.round(x * 32767.0).astype(np.int16)
    xq = q.astype(np.float32) / np.float32(32768.0)
    long = enveloped_noise(158403, 901)                # 3.3 s and a tail: 33 sub-blocks, so the short-term window is full
    want = {}
    for name, s in (("x", x), ("xq", xq), ("long", long)):
        E = ld.kweight_energies(s)
        ms, counts = ld.gate(E)
        one_shot = ld.loudness_ms_batch([s])
        assert same_bits(one_shot[0][0], ms)
        want[name] = (E, ld.lufs_of(ms), counts.tolist(), ld.momentary_of(E), ld.short_term_of(E))

    def check(meter, name):
        E, lufs, counts, mom, short = want[name]
        got, got_counts = meter.integrated(return_counts=True)
        assert same_bits(meter.energies(), E) and same_bits(got, lufs) and got_counts.tolist() == counts
        assert same_bits(meter.momentary(), mom) and same_bits(meter.short_term(), short)

    for sizes in ((4799,), (4800,), (7001,), (1, 4799, 4800, 7001), (len(x),)):
        check(feed(ld.LoudnessMeter(), x, sizes), "x")
    ones = ld.LoudnessMeter()                          # the first sub-block and one sample more, a sample at a time
    feed(ones, x[:4801], (1,))
    assert ones.energies().shape == (1,) and math.isnan(ones.integrated())
    check(feed(ones, x[4801:], (7001,)), "x")
    check(feed(ld.LoudnessMeter(), torch.from_numpy(x).cuda(), (7001,)), "x")
    check(feed(ld.LoudnessMeter(), q, (4799, 1, 7001)), "xq")              # an int16 feed
    assert math.isnan(want["x"][4]) and math.isfinite(want["long"][4])
    check(feed(ld.LoudnessMeter(), long, (7001,)), "long")
    # two meters interleaved do not disturb each other
    a, b = ld.LoudnessMeter(), ld.LoudnessMeter()
    for i in range(0, len(long), 7001):
        a.push(x[i:i + 7001])
        b.push(long[i:i + 7001])
    check(a, "x")
    check(b, "long")
    with pytest.raises(TypeError):
        a.push(np.zeros(10, np.float64))


@pytest.mark.parametrize("sr", [16000, 44100])
def test_other_rates_are_resampled_on_the_device_first(ld, sr):
    from flowdec_amd.resample import resample_device
    x = enveloped_noise(int(1.2 * sr) + 17, 950 + sr % 7)
    up = resample_device(torch.from_numpy(x).cuda(), sr, 48000, lowpass_filter_width=64).cpu().numpy()
    E = ld.kweight_energies(up)
    ms_want, counts_want = ld.gate(E)
    ms, counts = ld.loudness_ms_batch([x, x[:sr // 2]], sr=sr)
    assert same_bits(ms[0], ms_want) and counts[0].tolist() == counts_want.tolist() and counts_want[0] >= 8
    assert same_bits(ld.energies_batch([x], sr=sr)[0], E)
    # the host resampler differs by float32 rounding of the FIR only
    assert abs(ld.loudness_batch([x], sr=sr)[0] - ld.integrated_loudness(x, sr)) < 1e-4


def test_a_rate_whose_bank_does_not_fit_is_refused(ld):
    with pytest.raises(ValueError, match="cap"):
        ld.loudness_batch([np.zeros(48000, np.float32)], sr=47999)


def test_edge_cases_in_a_batch_leave_their_neighbours_alone(ld, clips, yard):
    good = [LENGTHS.index(n) for n in (24000, 48000, 100003)]
    bad_nan = clips[good[1]].copy()
    bad_nan[30000] = np.nan
    bad_inf = clips[good[1]].copy()
    bad_inf[100] = np.inf
    batch = [clips[good[0]], bad_nan, clips[good[1]], np.zeros(48000, np.float32), clips[LENGTHS.index(19199)], clips[good[2]], bad_inf,
             np.zeros(0, np.float32)]
    lufs, counts = ld.loudness_batch(batch, batch=8, return_counts=True)
    assert math.isnan(lufs[1]) and lufs[3] == float("-inf") and math.isnan(lufs[4]) and math.isnan(lufs[6]) and math.isnan(lufs[7])
    assert counts[1].tolist() == [7, 0, 0] and counts[3].tolist() == [7, 0, 0] and counts[4].tolist() == [0, 0, 0] == counts[7].tolist()
    for pos, k in zip((0, 2, 5), good):
        assert same_bits(lufs[pos], ld.lufs_of(yard[k][1])) and counts[pos].tolist() == yard[k][2].tolist()
    # the energies in front of the NaN are the clean clip's
    E = ld.energies_batch([bad_nan])[0]
    assert same_bits(E[:6], yard[good[1]][0][:6]) and np.all(np.isnan(E[6:]))


def test_refusals_leave_a_message_and_the_outputs_untouched(ld):
    from flowdec_amd import _lib as L
    lib = L.load()
    rows, lens = raw_rows([enveloped_noise(24000, 1)], 24000)
    nws = lib.fd_loudness_workspace_bytes(1, 24000)
    ws = torch.empty(nws, dtype=torch.uint8, device="cuda")
    ms = torch.full((1,), 7.0, dtype=torch.float64, device="cuda")
    counts = torch.full((1, 3), -1, dtype=torch.int32, device="cuda")
    E = torch.full((1, 5), 7.0, dtype=torch.float64, device="cuda")
    nsub = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    err = lambda: lib.fd_last_error().decode()
    assert lib.fd_loudness(L.ptr(rows), L.ptr(lens), 1, 24000, L.ptr(ms), L.ptr(counts), L.ptr(ws), nws - 1, L.stream()) == FD_ENOMEM
    assert "fd_loudness" in err() and "workspace" in err()
    assert lib.fd_loudness(L.ptr(rows), L.ptr(lens), 0, 24000, L.ptr(ms), L.ptr(counts), L.ptr(ws), nws, L.stream()) == FD_EINVAL and "B 0" in err()
    assert lib.fd_loudness(L.ptr(rows), None, 1, 24000, L.ptr(ms), L.ptr(counts), L.ptr(ws), nws, L.stream()) == FD_EINVAL and "null pointer" in err()
    assert lib.fd_loudness_energies(L.ptr(rows), L.ptr(lens), 1, 0, None, L.ptr(E), L.ptr(nsub), L.ptr(ws), nws, L.stream()) == FD_EINVAL and "L 0" in err()
    assert lib.fd_loudness_energies(L.ptr(rows), L.ptr(lens), 1, 24000, None, L.ptr(E), L.ptr(nsub), L.ptr(ws), 8, L.stream()) == FD_ENOMEM
    assert lib.fd_loudness_gate(L.ptr(E), L.ptr(nsub), 1, -1, L.ptr(ms), L.ptr(counts), L.stream()) == FD_EINVAL and "Jmax -1" in err()
    assert lib.fd_loudness_gate(L.ptr(E), L.ptr(nsub), 1, 5, None, L.ptr(counts), L.stream()) == FD_EINVAL and "null pointer" in err()
    torch.cuda.synchronize()
    assert ms.item() == 7.0 and counts.tolist() == [[-1, -1, -1]] and E.tolist() == [[7.0] * 5] and nsub.item() == -1
    # and the same buffers are written by a call that is taken
    L.check(lib.fd_loudness(L.ptr(rows), L.ptr(lens), 1, 24000, L.ptr(ms), L.ptr(counts), L.ptr(ws), nws, L.stream()))
    torch.cuda.synchronize()
    assert ms.item() != 7.0 and counts[0, 0].item() == 2


def test_eval_cli_on_the_gpu(ld, tmp_path, capsys):
    from flowdec_amd import eval_cli
    lst, _ = loudness_triples(tmp_path)
    G, H = eval_cli.GPU_SCORER, eval_cli.HOST_SCORER
    outs = {}
    for name, scorer, flags in (("gpu", G, ["--loudness", "--match-loudness"]), ("host", H, ["--loudness", "--match-loudness"]), ("plain", G, []),
                                ("before", eval_cli.Scorer(G.si_sxr, G.logspec, G.estoi, G.spectral, G.align, G.align_frac, G.shift), [])):
        out = tmp_path / f"{name}.csv"
        res = eval_cli.run(["--triples", str(lst), "--out", str(out), "--batch-files", "4"] + flags, scorer=scorer)
        assert res.exit_code == 0 and res.n_scored == 6
        outs[name] = (out, capsys.readouterr())
    hg, rg = read_csv(outs["gpu"][0])
    hh, rh = read_csv(outs["host"][0])
    assert hg == hh and tuple(hg[-3:]) == eval_cli.LUFS_NAMES
    for i, (a, b) in enumerate(zip(rg, rh)):
        for u, v in zip(a[-3:], b[-3:]):
            assert (u == v == "nan") if i == SHORT else abs(float(u) - float(v)) <= REF_BOUND_DB, (i, u, v)
        if i != SHORT:
            assert abs(float(a[7]) - float(b[7])) < 1e-2 * max(1.0, float(b[7]))          # logspec_mse after matching, GPU against host
    assert outs["gpu"][1].err.count("no loudness to match") == 2
    # without the flags: every byte is what a scorer without the new field writes
    assert outs["plain"][0].read_bytes() == outs["before"][0].read_bytes()
    assert outs["plain"][1].out.replace("plain.csv", "x.csv") == outs["before"][1].out.replace("before.csv", "x.csv") and "lufs" not in outs["plain"][1].out
