"""The corpus behind golden g32_estimate_params.npz (tests/golden/make_golden_estimate.py made the fixture from it; test_estimate_host.py and
test_hip_estimate.py rebuild it and check the hashes): 12 (clean, coded) pairs of PCM16 mono 48 kHz wavs and their pairs file.

Every sample comes from INTEGER arithmetic only -- a seeded RandomState.randint, integer moving sums (differences of an integer cumsum)
and shifts -- so the bytes are the same on every machine.  The files are written with the stdlib `wave` module.

* clean x: white integers through a moving sum of a pair-dependent width (a low-pass of a different corner per pair), shifted down to a
  pair-dependent level; lengths spread over 1.0 .. 3.2 s, one of exactly 96000 samples, one of 96001 (the crop start can only be 0),
  five shorter (zero-padded by the estimator) and five longer (cropped at a drawn start).
* coded y: x plus band-shaped integer noise (the first difference of a moving sum: a band-pass whose centre moves with the pair), at a
  level that moves with the pair.  Pairs 3 and 9 have a y that is LONGER than x (cut to x's length by the estimator)."""
import hashlib
import os
import wave

import numpy as np

SR = 48000
SEED = 3232
X_LENGTHS = [48000, 60000, 75000, 90001, 96000, 96001, 100000, 115200, 120007, 134400, 150000, 153600]
Y_EXTRA = {3: 1234, 9: 4800}            # pairs whose coded file is longer than the clean one
DELIM = " ---> "


def moving_sum(v: np.ndarray, width: int) -> np.ndarray:
    """out[i] = v[i] + ... + v[i + width - 1] (int64, exact)."""
    c = np.concatenate([[0], np.cumsum(v, dtype=np.int64)])
    return c[width:] - c[:-width]


def make_pair(i: int):
    """-> (x, y) int16 arrays of pair i."""
    rs = np.random.RandomState(SEED + i)
    n, ny = X_LENGTHS[i], X_LENGTHS[i] + Y_EXTRA.get(i, 0)
    wx = 4 + 3 * (i % 4)                                    # 4, 7, 10, 13 taps
    x = moving_sum(rs.randint(-4096, 4096, n + wx - 1).astype(np.int64), wx) >> (2 + i % 3)
    wn = 2 + i % 5                                          # 2 .. 6 taps, then a first difference
    e = moving_sum(rs.randint(-2048, 2048, ny + wn).astype(np.int64), wn)
    e = (e[1:] - e[:-1]) >> (2 + (i // 2) % 3)
    y = e.copy()
    y[:n] += x
    return np.clip(x, -32768, 32767).astype(np.int16), np.clip(y, -32768, 32767).astype(np.int16)


def write_wav(path: str, samples: np.ndarray) -> None:
    with wave.open(path, "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(SR)
        w.writeframes(samples.astype("<i2").tobytes())


def names(i: int):
    return f"clean_{i:02d}.wav", f"coded_{i:02d}.wav"


def build(directory: str) -> str:
    """Writes the 24 wavs and `pairs.txt` (absolute paths, one pair per line, in index order) into `directory` -> the pairs file."""
    os.makedirs(directory, exist_ok=True)
    lines = []
    for i in range(len(X_LENGTHS)):
        x, y = make_pair(i)
        px, py = (os.path.join(directory, nm) for nm in names(i))
        write_wav(px, x)
        write_wav(py, y)
        lines.append(px + DELIM + py)
    pairs = os.path.join(directory, "pairs.txt")
    with open(pairs, "w") as f:
        f.write("\n".join(lines) + "\n")
    return pairs


def hashes(directory: str):
    """-> sha256 hex digests of the 24 wav files, clean then coded per pair, in index order."""
    out = []
    for i in range(len(X_LENGTHS)):
        for nm in names(i):
            with open(os.path.join(directory, nm), "rb") as f:
                out.append(hashlib.sha256(f.read()).hexdigest())
    return out


def printed_numbers(lines):
    """The numbers of the estimator's result lines as printed: every `= 1.234` / `beta=0.36` (a path behind `sigma_y=<written to` has none)."""
    import re
    return [m for l in lines for m in re.findall(r"=\s*(-?[0-9]+\.[0-9]+|nan|inf)", l.split("<written to")[0])]
