"""csrc/stoi.hip -- ESTOI over ragged batches (include/flowdec_hip.h "ESTOI"; flowdec_amd/metrics.py estoi_batch; eval_cli --estoi) --
against the host function flowdec_amd.metrics.estoi (NumPy float64).  Parity with the pystoi package is unpinned (tests/test_estoi_cpu.py).

The clips: seeded noise under a slow envelope with a gate (test_estoi_cpu.gated_clip), 0.5 - 1.2 s, five at 16 kHz (one of them 0.4 s: too
short), five at 48 kHz, one at 10 kHz (no resample plan).  The metric is discontinuous where a frame's energy sits on the 40 dB
threshold, and the kernel reads float32-rounded resampled samples: the fixture asserts ON THE HOST that every frame of every clip is at
least 1e-3 dB from the threshold (six orders above what float32 rounding moves an energy by) and takes the next seed otherwise.

(1) Mask and compaction: kept_out and frames_out equal the host function's lists (integers).
(2) Band magnitudes within a derived bound of float64.  The float64 side starts from the float32 samples the kernel's resampler produces
    (fd_resample's arithmetic on the host: float32 bank, float64 sums, one rounding).  Per DFT component of a frame z (256 samples, S = sum
    |z_n|): z_n is rounded once to float32 (u = 2^-24), may differ by one more float32 place where the host's float64 sum of the resampler
    rounds the other way (2 u), the table entry carries one rounding (u), the product one and the 255 additions of the fma chain 255 u of
    the sum of |terms|, |terms| <= |z_n|: (K + 4) u S to first order, below E = C_BOUND K u S with test_hip_stft.py's C_BOUND = 2 and
    K = 256.  Then P = re^2 + im^2 in float32: |dP| <= 2 E (|Re| + |Im|) + 2 E^2 + 3 u P' (two products, one sum; P' the perturbed value);
    the band sum S_b in float64 adds nothing visible (15 2^-53); |sqrt(a) - sqrt(b)| <= min(|a - b| / sqrt(b), sqrt|a - b|); the last
    rounding to float32 adds u of the value.
(3) ESTOI against the host function.  The tolerance is measured on the host, never from the kernel: the host function's float32 mode
    rounds where the kernel rounds (resampled signal, |X|^2, band magnitude); the kernel also accumulates its DFT in float32 over 256
    terms, so the bound is 16 (= sqrt 256) times the largest |float32 mode - float64 mode| over the test clips (those of (8) included).
    That bound must itself be at most 1e-5.
(4) estoi(x, x) within 1e-6 of 1; estoi(x, 4 y) == estoi(x, y) bit for bit.
(5) Batch invariance bit for bit: alone == in a ragged batch of five at the first, middle and last position (NaN behind every clip's
    end); estoi_batch with batch = 2 gives the same bits.
(6) The 0.4 s clip: 1e-5, fewer than 30 spectral frames, neighbours unchanged.
(7) Refusals: FD_EINVAL with a message, outputs untouched.
(8) eval_cli --estoi on six WAV triples: the estoi column within (3)'s bound of HOST_SCORER's, the other columns byte-identical to a run
    without the flag."""
import ctypes as C

import numpy as np
import pytest
import torch

from test_estoi_cpu import gated_clip, make_triples, noisy
from test_eval_cpu import read_csv
from test_hip_stft import C_BOUND, U, dev

pytestmark = pytest.mark.gpu

FD_EINVAL = -1
MARGIN_DB = 1e-3
SPECS = {16000: [0.4, 0.65, 0.5, 1.0, 1.2], 48000: [0.7, 0.5, 1.2, 0.9, 1.05], 10000: [1.0]}
SNRS = [30, 10, 0, -10, 5]
SHORT = (16000, 0)          # the 0.4 s clip


def L_():
    from flowdec_amd import _lib
    return _lib


def lib():
    return L_().load()


def M_():
    from flowdec_amd import metrics
    return metrics


class Clip:
    def __init__(self, sr, dur, snr, seed0):
        m = M_()
        for seed in range(seed0, seed0 + 50):
            self.x = gated_clip(sr, dur, seed)
            if m.estoi_detail(self.x, self.x, sr)["margin_db"] >= MARGIN_DB:
                break
        else:
            raise AssertionError("no seed keeps every frame 1e-3 dB from the threshold")
        self.sr, self.seed = sr, seed
        self.h = noisy(self.x, snr, seed + 1000)
        self.d64 = m.estoi_detail(self.h, self.x, sr)
        assert self.d64["margin_db"] >= MARGIN_DB
        self.v32 = m.estoi(self.h, self.x, sr, precision="float32")


@pytest.fixture(scope="module")
def clips():
    out = {sr: [Clip(sr, d, SNRS[i], 100 * i + sr % 97) for i, d in enumerate(durs)] for sr, durs in SPECS.items()}
    for sr, cs in out.items():
        for i, c in enumerate(cs):
            assert c.d64["too_short"] == ((sr, i) == SHORT), (sr, i, c.d64["spectral_frames"])
            assert np.any(np.diff(c.d64["kept"]) > 1)                       # kept frames are not adjacent at the source
    return out


def rows_of(sigs, Lrow=None):
    """[B, Lrow] float32 rows, NaN behind every clip's end: a read there poisons the result."""
    Lrow = Lrow or max(len(s) for s in sigs)
    r = np.full((len(sigs), Lrow), np.nan, np.float32)
    for b, s in enumerate(sigs):
        r[b, :len(s)] = s
    return r


def call(sr, hs, xs, bands=False, Lrow=None):
    """One ragged call -> (estoi [B] float64, frames [B, 3]) or, bands=True, (frames, kept [B, T_max], tob [B, 2, T_max, 15])."""
    l, m = L_(), M_()
    plans = m.estoi_plans(sr)
    h, x = dev(rows_of(hs, Lrow)), dev(rows_of(xs, Lrow))
    lens = torch.tensor([len(s) for s in xs], dtype=torch.int32, device="cuda")
    B, Lr = x.shape
    nws = lib().fd_metrics_estoi_workspace_bytes(B, Lr, plans.o, plans.n)
    ws = torch.empty(nws, dtype=torch.uint8, device="cuda")
    fr = torch.full((B, 3), -7, dtype=torch.int32, device="cuda")
    if not bands:
        val = torch.full((B,), 7.0, dtype=torch.float64, device="cuda")
        l.check(lib().fd_metrics_estoi(plans.estoi, plans.resample, l.ptr(h), l.ptr(x), l.ptr(lens), B, Lr, l.ptr(val), l.ptr(fr), l.ptr(ws), nws, l.stream()))
        return val.cpu().numpy(), fr.cpu().numpy()
    Tm = lib().fd_metrics_estoi_max_frames(Lr, plans.o, plans.n)
    kept = torch.full((B, Tm), -7, dtype=torch.int32, device="cuda")
    tob = torch.full((B, 2, Tm, 15), 7.0, dtype=torch.float32, device="cuda")
    l.check(lib().fd_metrics_estoi_bands(plans.estoi, plans.resample, l.ptr(h), l.ptr(x), l.ptr(lens), B, Lr, l.ptr(fr), l.ptr(kept), l.ptr(tob),
                                         l.ptr(ws), nws, l.stream()))
    return fr.cpu().numpy(), kept.cpu().numpy(), tob.cpu().numpy()


@pytest.fixture(scope="module")
def batch_results(clips):
    """Every rate's clips in ONE ragged call each: (estoi, frames) and the stage outputs; shared by the tests below."""
    out = {}
    for sr, cs in clips.items():
        hs, xs = [c.h for c in cs], [c.x for c in cs]
        out[sr] = (call(sr, hs, xs), call(sr, hs, xs, bands=True))
    return out


@pytest.fixture(scope="module")
def bound(clips, tmp_path_factory):
    """(3)'s tolerance: 16 x the largest |float32 mode - float64 mode| of the host function over the test clips, those of (8) included."""
    from flowdec_amd.eval_cli import load_mono
    m = M_()
    diffs = [abs(c.v32 - c.d64["value"]) for cs in clips.values() for c in cs]
    tmp = tmp_path_factory.mktemp("estoi_triples")
    lst, _ = make_triples(tmp, [0.5, 0.7, 0.4, 1.2, 0.9, 0.6], sr=16000, seed=7)
    for line in open(lst).read().split("\n"):
        if line:
            xp, _, hp = line.split(" ---> ")
            h, x = load_mono(hp, 16000).numpy(), load_mono(xp, 16000).numpy()
            diffs.append(abs(m.estoi(h, x, 16000, precision="float32") - m.estoi(h, x, 16000)))
    b = 16 * max(diffs)
    print(f"|f32 mode - f64 mode| of the host function: {min(d for d in diffs if d > 0):.3g} .. {max(diffs):.3g}; bound {b:.3g}")
    assert 0 < b <= 1e-5
    return b, lst, tmp


def test_mask_and_compaction_equal_the_host_lists(clips, batch_results):
    for sr, cs in clips.items():
        fr, kept, _ = batch_results[sr][1]
        for b, c in enumerate(cs):
            d = c.d64
            k = len(d["kept"])
            assert fr[b].tolist() == [d["frames"], k, d["spectral_frames"]], (sr, b)
            assert np.array_equal(kept[b, :k], d["kept"]) and (kept[b, k:] == -1).all(), (sr, b)
            assert k < d["frames"]                                            # the gate removed frames


def test_band_magnitudes_within_the_derived_bound(clips, batch_results):
    m = M_()
    worst = 0.0
    for sr, cs in clips.items():
        _, _, tob = batch_results[sr][1]
        for b, c in enumerate(cs):
            if sr == 10000:
                x10, h10 = c.x, c.h
            else:
                bank, o, n, width = m.estoi_bank(sr)
                x10, h10 = (m.polyphase_resample(s, bank, o, n, width).astype(np.float32) for s in (c.x, c.h))
            d = m.estoi_detail(h10, x10, 10000, keep_spectra=True)
            assert np.array_equal(d["kept"], c.d64["kept"])
            T = d["spectral_frames"]
            assert (tob[b, :, T:] == 0).all()
            for s, (tk, Xk, ak) in enumerate((("tob_x", "spec_x", "abs1_x"), ("tob_x_hat", "spec_x_hat", "abs1_x_hat"))):
                ref, X, S = d[tk], d[Xk], d[ak]
                E = (C_BOUND * 256 * U * S)[:, None]
                re, im = np.abs(X.real), np.abs(X.imag)
                dP = 2 * E * (re + im) + 2 * E * E
                dP = dP + 3 * U * (re * re + im * im + dP)
                bnd = np.zeros_like(ref)
                for i, (lo, hi) in enumerate(m.estoi_band_edges()):
                    dS = dP[:, lo:hi].sum(axis=1) * (1 + 2.0 ** -48)
                    root = np.minimum(dS / np.maximum(ref[:, i], 1e-300), np.sqrt(dS))
                    bnd[:, i] = root + U * (ref[:, i] + root)
                err = np.abs(tob[b, s, :T].astype(np.float64) - ref)
                bad = np.argwhere(~(err <= bnd))
                assert bad.size == 0, f"sr {sr} clip {b} signal {s}: {len(bad)} magnitudes over the bound, first {bad[0].tolist()}: {err[tuple(bad[0])]:.3e} > {bnd[tuple(bad[0])]:.3e}"
                worst = max(worst, float((err / bnd).max()))
    print(f"band magnitudes: max error / bound {worst:.3g}")


def test_estoi_within_the_measured_bound_of_the_host_function(clips, batch_results, bound):
    tol = bound[0]
    worst = 0.0
    for sr, cs in clips.items():
        val, _ = batch_results[sr][0]
        for b, c in enumerate(cs):
            diff = abs(val[b] - c.d64["value"])
            print(f"sr {sr} clip {b}: gpu {val[b]:.12f} host {c.d64['value']:.12f} diff {diff:.3g} (f32 mode diff {abs(c.v32 - c.d64['value']):.3g})")
            worst = max(worst, diff)
    print(f"largest |gpu - host float64| {worst:.3g}, bound {tol:.3g}")
    assert worst <= tol


def test_identity_and_power_of_two_scale(clips):
    for sr, cs in clips.items():
        xs = [c.x for c in cs if not c.d64["too_short"]]
        hs = [c.h for c in cs if not c.d64["too_short"]]
        same, _ = call(sr, xs, xs)
        assert np.abs(same - 1.0).max() <= 1e-6, same
        a, fa = call(sr, hs, xs)
        b, fb = call(sr, [4 * h for h in hs], xs)
        assert a.tobytes() == b.tobytes() and np.array_equal(fa, fb)


def test_batch_invariance_bit_for_bit(clips, batch_results):
    m = M_()
    for sr in (16000, 48000):
        cs = clips[sr]
        ref, ref_fr = batch_results[sr][0]
        for i, c in enumerate(cs):
            alone, fr = call(sr, [c.h], [c.x])
            assert alone.tobytes() == ref[i:i + 1].tobytes() and np.array_equal(fr[0], ref_fr[i]), (sr, i)
            others = [j for j in range(len(cs)) if j != i]
            for pos in (0, 2, 4):
                order = others[:pos] + [i] + others[pos:]
                v, f = call(sr, [cs[j].h for j in order], [cs[j].x for j in order])
                assert v[pos:pos + 1].tobytes() == alone.tobytes() and np.array_equal(f[pos], fr[0]), (sr, i, pos)
                assert v.tobytes() == ref[order].tobytes()
        v2, f2 = m.estoi_batch([torch.from_numpy(c.h) for c in cs], [torch.from_numpy(c.x) for c in cs], sr=sr, batch=2, return_frames=True)
        assert v2.tobytes() == ref.tobytes() and np.array_equal(f2, ref_fr)
    # a longer row than any clip needs changes nothing either
    c = clips[10000][0]
    a, _ = call(10000, [c.h], [c.x])
    b, _ = call(10000, [c.h], [c.x], Lrow=len(c.x) + 1000)
    assert a.tobytes() == b.tobytes() == batch_results[10000][0][0].tobytes()


def test_short_clip_gives_pystois_value_and_leaves_its_neighbours(clips, batch_results):
    sr, i = SHORT
    val, fr = batch_results[sr][0]
    assert val[i] == 1e-5 and 0 < fr[i, 2] < 30 and fr[i, 2] == clips[sr][i].d64["spectral_frames"]
    rest = [j for j in range(len(clips[sr])) if j != i]
    v, f = call(sr, [clips[sr][j].h for j in rest], [clips[sr][j].x for j in rest])
    assert v.tobytes() == val[rest].tobytes() and np.array_equal(f, fr[rest])
    # 200 samples: no frame at all
    v, f = call(sr, [clips[sr][0].h[:200]], [clips[sr][0].x[:200]])
    assert v[0] == 1e-5 and f[0].tolist() == [0, 0, 0]


def test_refusals_leave_the_outputs_untouched(clips):
    l, m = L_(), M_()
    plans = m.estoi_plans(16000)
    c = clips[16000][1]
    h, x = dev(rows_of([c.h])), dev(rows_of([c.x]))
    lens = torch.tensor([len(c.x)], dtype=torch.int32, device="cuda")
    Lr = len(c.x)
    nws = lib().fd_metrics_estoi_workspace_bytes(1, Lr, plans.o, plans.n)
    ws = torch.empty(nws, dtype=torch.uint8, device="cuda")
    val = torch.full((1,), 7.0, dtype=torch.float64, device="cuda")
    fr = torch.full((1, 3), -7, dtype=torch.int32, device="cuda")
    err = lambda: lib().fd_last_error().decode()
    args = lambda **kw: [kw.get("plan", plans.estoi), plans.resample, kw.get("h", l.ptr(h)), l.ptr(x), l.ptr(lens), kw.get("B", 1), Lr, l.ptr(val), l.ptr(fr),
                         l.ptr(ws), kw.get("nws", nws), l.stream()]
    assert lib().fd_metrics_estoi(*args(plan=None)) == FD_EINVAL and "null pointer" in err()
    assert lib().fd_metrics_estoi(*args(h=None)) == FD_EINVAL and "null pointer" in err()
    assert lib().fd_metrics_estoi(*args(nws=nws - 1)) == FD_EINVAL and "workspace too small" in err()
    assert lib().fd_metrics_estoi(*args(B=0)) == FD_EINVAL and "bad batch B 0" in err()
    torch.cuda.synchronize()
    assert val.item() == 7.0 and (fr == -7).all()
    assert lib().fd_metrics_estoi(*args()) == 0
    assert val.item() == pytest.approx(c.d64["value"], abs=1e-5)


def test_eval_cli_estoi_on_wav_triples(bound):
    from flowdec_amd import eval_cli
    tol, lst, tmp = bound
    base, gpu, host = tmp / "base.csv", tmp / "gpu.csv", tmp / "host.csv"
    common = ["--triples", str(lst), "--sr", "16000", "--batch-files", "4"]
    r0 = eval_cli.run(common + ["--out", str(base)])
    r1 = eval_cli.run(common + ["--out", str(gpu), "--estoi"])
    eval_cli.run(common + ["--out", str(host), "--estoi"], scorer=eval_cli.HOST_SCORER)
    h0, rows0 = read_csv(base)
    h1, rows1 = read_csv(gpu)
    _, rowsh = read_csv(host)
    assert tuple(h0) == eval_cli.CSV_HEADER and h1 == h0 + ["estoi"] and len(rows1) == 6
    assert [r[:8] for r in rows1] == rows0 and r1.means[:4] == r0.means and r1.means[4][0] == "estoi"
    g, h = np.array([float(r[8]) for r in rows1]), np.array([float(r[8]) for r in rowsh])
    print(f"eval_cli --estoi: largest |gpu - host| {np.abs(g - h).max():.3g}, bound {tol:.3g}; values {g}")
    assert np.abs(g - h).max() <= tol
    assert rows1[2][8] == "1e-05" == rowsh[2][8]                              # the 0.4 s triple
    assert r1.means[4][2] == 6
