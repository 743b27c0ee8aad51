"""Shared inputs of tests/test_loudness_cpu.py and tests/test_hip_loudness.py: an independent BS.1770 reading built on scipy.signal.lfilter
and literal loops, the seeded signals, and the six WAV triples of the command-line tests.  No test lives here."""
import numpy as np

SR = 48000
SUB = 4800
# lengths of the independent-reference inputs: exactly one block, one block and a sub-block, 1 s, a ragged tail, 30 s
REF_LENGTHS = (19200, 24000, 48000, 100003, 30 * SR)
# |LUFS(yardstick) - LUFS(lfilter reference)| over the REF_LENGTHS inputs below measured 1.25e-14 dB at the most on the host (the two
# differ only in the order of float64 additions and in the chunked carry); the tests allow 16 x that.  A changed summation order moves the
# value by about 1e-13 dB at the most, a wrong coefficient or gate by more than 1e-3 dB.
REF_MAX_OBSERVED_DB = 1.25e-14
REF_BOUND_DB = 16 * REF_MAX_OBSERVED_DB
assert REF_BOUND_DB < 1e-9


def reference_reading(x, K48, abs_gate):
    """-> (LUFS, counts[3], E, ms): scipy.signal.lfilter in float64, then literal loops over sub-blocks and blocks."""
    from scipy.signal import lfilter
    z = np.asarray(x, np.float32).astype(np.float64)
    for b0, b1, b2, a1, a2 in K48:
        z = lfilter([b0, b1, b2], [1.0, a1, a2], z)
    nsub = len(z) // SUB
    E = np.zeros(nsub)
    for j in range(nsub):
        E[j] = float(np.sum(np.square(z[SUB * j:SUB * (j + 1)])))
    ms = np.zeros(max(nsub - 3, 0))
    for j in range(len(ms)):
        ms[j] = (E[j] + E[j + 1] + E[j + 2] + E[j + 3]) / 19200.0
    if len(ms) == 0:
        return float("nan"), np.array([0, 0, 0]), E, ms
    above = [m for m in ms if m > abs_gate]
    if not above:
        return float("-inf"), np.array([len(ms), 0, 0]), E, ms
    thr = 0.1 * (sum(above) / len(above))
    both = [m for m in above if m > thr]
    return -0.691 + 10 * np.log10(sum(both) / len(both)), np.array([len(ms), len(above), len(both)]), E, ms


def gate_margins(ms, abs_gate):
    """The smallest relative distance of any block's mean square from the absolute and from the relative threshold."""
    if len(ms) == 0:
        return np.inf
    above = ms[ms > abs_gate]
    d = np.min(np.abs(ms - abs_gate) / abs_gate)
    if len(above):
        thr = 0.1 * above.mean()
        d = min(d, np.min(np.abs(ms - thr) / thr))
    return d


def enveloped_noise(n, seed):
    """Seeded noise under an envelope: a loud first part, a stretch of digital silence, then a half that is 30 dB down (below the relative
    gate once the loud part sets it), with a slow swell so that no two blocks are alike."""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / n
    env = np.where(t < 0.4, 0.2, np.where(t < 0.5, 0.0, 0.2 * 10 ** (-30 / 20)))
    env = env * (1.0 + 0.5 * np.sin(2 * np.pi * 3 * t))
    return (env * rng.standard_normal(n)).astype(np.float32)


def reference_inputs(K48, abs_gate):
    """One signal per REF_LENGTHS entry whose every block lies at least 1e-6 (relative) away from both gate thresholds -- so that no
    rounding decides a comparison -- taking the next seed otherwise.  -> [(x, LUFS, counts)]."""
    out = []
    for k, n in enumerate(REF_LENGTHS):
        for seed in range(100 * k, 100 * k + 20):
            x = enveloped_noise(n, seed)
            lufs, counts, _, ms = reference_reading(x, K48, abs_gate)
            if gate_margins(ms, abs_gate) >= 1e-6:
                break
        else:
            raise AssertionError(f"no seed keeps the blocks of a {n}-sample input away from the gates")
        assert gate_margins(ms, abs_gate) >= 1e-6
        out.append((x, lufs, counts))
    return out


def tone(freq, dbfs_and_seconds, sr=SR):
    """A sine of `freq` Hz whose peak level steps through (dBFS, seconds) pairs, phase continuous."""
    amps = np.concatenate([np.full(int(round(sec * sr)), 10 ** (db / 20)) for db, sec in dbfs_and_seconds])
    return (amps * np.sin(2 * np.pi * freq * np.arange(len(amps)) / sr)).astype(np.float32)


QUIET_DB = {1: -6.0, 3: -2.5}     # triple -> the level of its x_hat and y against the others
SHORT = 5                         # the triple under 400 ms
TRIPLE_SAMPLES = (24000, 30000, 24000, 28803, 19200, 6000)


def loudness_triples(tmp_path, sr=SR):
    """Six float32 WAV triples: 1 and 3 have x_hat and y 6 dB and 2.5 dB quiet, 5 is shorter than 400 ms.  -> (list file, signals)."""
    import torch
    from flowdec_amd.audio import save_wav
    rng = np.random.default_rng(2024)
    lines, sigs = [], []
    for i, n in enumerate(TRIPLE_SAMPLES):
        x = (0.1 * rng.standard_normal(n)).astype(np.float32)
        y = x + (0.03 * rng.standard_normal(n)).astype(np.float32)
        h = x + (0.003 * rng.standard_normal(n)).astype(np.float32)
        g = np.float32(10 ** (QUIET_DB.get(i, 0.0) / 20))
        h, y = h * g, y * g
        paths = [tmp_path / f"clean_{i}.wav", tmp_path / f"noisy_{i}.wav", tmp_path / f"enh_{i}.wav"]
        for p, s in zip(paths, (x, y, h)):
            save_wav(str(p), torch.from_numpy(s), sr)
        lines.append(" ---> ".join(str(p) for p in paths))
        sigs.append((h, x, y))
    lst = tmp_path / "loud_triples.txt"
    lst.write_text("\n".join(lines) + "\n")
    return lst, sigs
