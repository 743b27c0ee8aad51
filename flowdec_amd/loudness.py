"""Integrated loudness after ITU-R BS.1770-4 / EBU R 128 (K-weighting, 400 ms blocks at 75 % overlap, the absolute and the relative gate)
of mono signals at 48 kHz: the host yardstick in NumPy float64, which is the definition, and the same arithmetic on the GPU over ragged
batches and streams (csrc/loudness.hip, include/flowdec_hip.h "Loudness").  eval_cli --loudness / --match-loudness use it to report the
level of x_hat, x and y and to undo a level difference before the metrics that are not scale-invariant.

The measure is a published standard: the coefficients K48 are Tables 1 and 2 of BS.1770-4, and the conformance readings of the standard
and of EBU Tech 3341 pin the host function (tests/test_loudness_cpu.py).  Parity with the `pyloudnorm` / `audiotools` packages is UNPINNED
(both absent offline; scripts/pin_loudness.py prints the difference where pyloudnorm is importable).

The definition, in the order of operations the device follows bit for bit (every product, sum, difference and quotient is one float64
operation rounded on its own; nothing is fused):

1. The step of the filter, transposed direct form II, the two biquads in cascade, on the state s = (s1, s2, s3, s4) (`_kstep`):
       y = B0 x + s1      s1' = (B1 x - A1 y) + s2      s2' = B2 x - A2 y            (stage 1, the shelf)
       z = y + s3         s3' = (D1 y - C1 z) + s4      s4' = y - C2 z               (stage 2, the high-pass: b = 1, -2, 1)
2. Only whole sub-blocks of SUB = 4800 samples, counted from sample 0, are read; the last n mod 4800 samples are not.  A sub-block is 64
   chunks of CHUNK = 75 samples.  M_CHUNK and M_SUB are the zero-input transitions over 75 and 4800 samples: column i is the state after
   that many steps with x = 0 from the unit state i (`transition`).  `e + M s` below means e_i + (((M_i0 s_0 + M_i1 s_1) + M_i2 s_2) +
   M_i3 s_3) (`_advance`).
3. Pass A: e_jk = the state after the 75 steps of chunk k of sub-block j from the zero state; T_j = t_64 of t_0 = 0, t_{k+1} = e_jk +
   M_CHUNK t_k.  Carry: S_0 = the state handed in (zeros), S_{j+1} = T_j + M_SUB S_j.  Pass B: s_j0 = S_j, s_{j,k+1} = e_jk + M_CHUNK s_jk;
   chunk k runs its 75 steps again from s_jk, adding z z in ascending sample order to 0.0; E[j] = the 64 chunk sums added in ascending k.
   (The carry is linear superposition: exact in real numbers, and against scipy.signal.lfilter the energies differ by about 1e-13
   relative.)
4. Gating block j is the sub-blocks j .. j + 3: ms_j = (((E[j] + E[j+1]) + E[j+2]) + E[j+3]) / 19200.  A sum over blocks is 64 lane sums
   (lane l adds its blocks l, l + 64, ... in ascending order to 0.0) added in ascending l (`_lane_sum`).  sum1, n1 over ms_j > ABS_GATE =
   10^((-70 + 0.691) / 10); thr = 0.1 * (sum1 / n1); sum2, n2 over ms_j > ABS_GATE and ms_j > thr; ms_gated = sum2 / n2.  Both gates
   compare mean squares: no logarithm decides a comparison.
5. Fewer than 19200 samples: NaN, counts (0, 0, 0).  A block that is NaN or Inf (a NaN or Inf sample in a sub-block that was read): NaN,
   counts (blocks, 0, 0); other clips of a batch are not touched.  No block above the absolute gate: ms_gated = 0.0, -inf LUFS.
6. LUFS = -0.691 + 10 log10(ms_gated) is formed here, in Python, also from the device's ms_gated (`lufs_of`).

Rates other than 48 kHz are brought there first with the project's own resampler at lowpass_filter_width=64 (`audio.resample` here,
`resample.resample_device` on the GPU); no coefficients are derived for other rates.  A rate whose filter bank is over the device
resampler's cap is refused.

The rest of an EBU R 128 meter is defined further down, in the same manner (a NumPy float64 yardstick whose order of operations the device
follows bit for bit; csrc/loudness_range.hip): loudness range after EBU Tech 3342 (`range_of`, `loudness_range`), true peak after BS.1770-4
Annex 2 (`true_peak_lin`, `true_peak`), the gain that brings a file to a target loudness under a true-peak ceiling (`output_gain`,
`normalize_loudness`; enhance_cli --target-lufs / --peak-ceiling) and the level of a file of several channels (`file_level`).
"""
import ctypes as C
import math

import numpy as np
import torch

from . import _lib as L
from . import align
from . import audio
from . import resample as fd_resample
from .batching import ragged_batches

SR = 48000
SUB = 4800                       # samples per sub-block: 100 ms
CHUNK = 75                       # samples per chunk: one lane of the kernel
NCHUNK = SUB // CHUNK            # 64
BLOCK_SUBS = 4                   # a gating block: 400 ms
SHORT_SUBS = 30                  # the short-term window: 3 s
MIN_SAMPLES = BLOCK_SUBS * SUB   # 19200
LANES = 64
RESAMPLE_WIDTH = 64              # lowpass_filter_width of the resampling in front of another rate

# ITU-R BS.1770-4 Table 1 (stage 1, the shelf) and Table 2 (stage 2, the high-pass) at 48 kHz: (b0, b1, b2, a1, a2)
K48 = ((1.53512485958697, -2.69169618940638, 1.19839281085285, -1.69065929318241, 0.73248077421585),
       (1.0, -2.0, 1.0, -1.99004745483398, 0.99007225036621))
ABS_GATE = 10.0 ** ((-70 + 0.691) / 10)     # mean square of -70 LUFS
REL_GATE = 0.1                              # -10 LU, on the mean square
(_B0, _B1, _B2, _A1, _A2), (_, _D1, _, _C1, _C2) = K48


def _kstep(x, s):
    """One step of the cascade on the state list s (four float64 arrays or scalars, replaced in place) -> z."""
    p = _B0 * x
    y = p + s[0]
    q1 = _B1 * x
    q2 = _A1 * y
    r = q1 - q2
    n1 = r + s[1]
    u1 = _B2 * x
    u2 = _A2 * y
    n2 = u1 - u2
    z = y + s[2]
    v1 = _D1 * y
    v2 = _C1 * z
    w = v1 - v2
    n3 = w + s[3]
    g = _C2 * z
    n4 = y - g
    s[0], s[1], s[2], s[3] = n1, n2, n3, n4
    return z


def _advance(M, e, s):
    """e + M s in the stated order; e and s are lists of four arrays (or scalars) -> the new list."""
    out = []
    for i in range(4):
        a = M[i, 0] * s[0]
        c = M[i, 1] * s[1]
        a = a + c
        c = M[i, 2] * s[2]
        a = a + c
        c = M[i, 3] * s[3]
        a = a + c
        out.append(e[i] + a)
    return out


def transition(steps: int) -> np.ndarray:
    """The zero-input transition over `steps` samples, float64 [4, 4]: column i is the state after `steps` steps with x = 0 from the
    unit state i."""
    s = [np.array([1.0 if r == c else 0.0 for c in range(4)], np.float64) for r in range(4)]      # s[r][c]: component r of column c
    zero = np.zeros(4, np.float64)
    for _ in range(int(steps)):
        _kstep(zero, s)
    return np.stack(s, axis=0)


M_CHUNK = transition(CHUNK)
M_SUB = transition(SUB)


def _samples(x) -> np.ndarray:
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().numpy()
    x = np.asarray(x).reshape(-1)
    if x.dtype != np.float32:
        raise TypeError(f"loudness: float32 samples (got {x.dtype})")
    return x


def kweight_energies(x, state=None, return_state: bool = False):
    """x float32 [n] at 48 kHz -> E float64 [n // 4800]: the energies of the K-weighted signal over its whole sub-blocks (steps 1 to 3 of
    the module docstring).  state: the filter state at sample 0 (float64 [4], default zeros); return_state: also the state after the
    last whole sub-block."""
    x = _samples(x)
    nsub = x.shape[0] // SUB
    S = [np.float64(v) for v in (np.zeros(4) if state is None else np.asarray(state, np.float64).reshape(4))]
    if nsub == 0:
        E = np.zeros(0, np.float64)
        return (E, np.array(S, np.float64)) if return_state else E
    X = x[:nsub * SUB].astype(np.float64).reshape(nsub, NCHUNK, CHUNK)
    with np.errstate(all="ignore"):
        s = [np.zeros((nsub, NCHUNK), np.float64) for _ in range(4)]
        for i in range(CHUNK):
            _kstep(X[:, :, i], s)
        e = s                                                        # e[i][j, k]
        t = [np.zeros(nsub, np.float64) for _ in range(4)]
        for k in range(NCHUNK):
            t = _advance(M_CHUNK, [e[i][:, k] for i in range(4)], t)
        starts = np.zeros((4, nsub), np.float64)                     # S_j
        for j in range(nsub):
            for i in range(4):
                starts[i, j] = S[i]
            S = _advance(M_SUB, [t[i][j] for i in range(4)], S)
        cur = [starts[i].copy() for i in range(4)]
        mine = [np.zeros((nsub, NCHUNK), np.float64) for _ in range(4)]
        for k in range(NCHUNK):
            for i in range(4):
                mine[i][:, k] = cur[i]
            cur = _advance(M_CHUNK, [e[i][:, k] for i in range(4)], cur)
        acc = np.zeros((nsub, NCHUNK), np.float64)
        for i in range(CHUNK):
            z = _kstep(X[:, :, i], mine)
            zz = z * z
            acc = acc + zz
        E = acc[:, 0].copy()
        for k in range(1, NCHUNK):
            E = E + acc[:, k]
    return (E, np.array(S, np.float64)) if return_state else E


def block_mean_squares(E) -> np.ndarray:
    """E [J] -> ms [max(J - 3, 0)]: (((E[j] + E[j+1]) + E[j+2]) + E[j+3]) / 19200."""
    E = np.asarray(E, np.float64).reshape(-1)
    if E.shape[0] < BLOCK_SUBS:
        return np.zeros(0, np.float64)
    with np.errstate(all="ignore"):
        a = E[:-3] + E[1:-2]
        a = a + E[2:-1]
        a = a + E[3:]
        return a / float(MIN_SAMPLES)


def _lane_sum(v: np.ndarray, keep: np.ndarray) -> np.float64:
    w = np.where(keep, v, 0.0)
    rows = np.concatenate([w, np.zeros(-len(w) % LANES, np.float64)]).reshape(-1, LANES)
    acc = np.zeros(LANES, np.float64)
    for r in rows:
        acc = acc + r
    total = acc[0]
    for l in range(1, LANES):
        total = total + acc[l]
    return total


def gate(E):
    """E float64 [J] -> (ms_gated float64, counts int32 [3] = blocks, blocks above the absolute gate, blocks above both): steps 4 and 5
    of the module docstring."""
    ms = block_mean_squares(E)
    nblk = ms.shape[0]
    if nblk == 0:
        return np.float64(np.nan), np.zeros(3, np.int32)
    if not np.all(np.isfinite(ms)):
        return np.float64(np.nan), np.array([nblk, 0, 0], np.int32)
    keep1 = ms > ABS_GATE
    n1 = int(np.count_nonzero(keep1))
    if n1 == 0:
        return np.float64(0.0), np.array([nblk, 0, 0], np.int32)
    thr = np.float64(REL_GATE) * (_lane_sum(ms, keep1) / np.float64(n1))
    keep2 = keep1 & (ms > thr)
    n2 = int(np.count_nonzero(keep2))
    return _lane_sum(ms, keep2) / np.float64(n2), np.array([nblk, n1, n2], np.int32)


def lufs_of(ms):
    """-0.691 + 10 log10(ms): a mean square (scalar or array) -> LUFS; 0 -> -inf, NaN -> NaN."""
    with np.errstate(divide="ignore", invalid="ignore"):
        out = -0.691 + 10.0 * np.log10(np.asarray(ms, np.float64))
    return float(out) if out.ndim == 0 else out


def _window_lufs(E, subs: int) -> float:
    E = np.asarray(E, np.float64).reshape(-1)
    if E.shape[0] < subs:
        return float("nan")
    with np.errstate(all="ignore"):
        a = E[-subs]
        for k in range(-subs + 1, 0):
            a = a + E[k]
        return lufs_of(a / float(subs * SUB))


def momentary_of(E) -> float:
    """The momentary loudness (400 ms, ungated) at the end of E: its last 4 sub-blocks added in ascending order; NaN for fewer."""
    return _window_lufs(E, BLOCK_SUBS)


def short_term_of(E) -> float:
    """The short-term loudness (3 s, ungated) at the end of E: its last 30 sub-blocks added in ascending order; NaN for fewer."""
    return _window_lufs(E, SHORT_SUBS)


def gain_db(l_from: float, l_to: float) -> float:
    """The gain in dB that brings a signal of loudness l_from to l_to."""
    return float(l_to) - float(l_from)


def gain_factor(l_from: float, l_to: float) -> np.float32:
    """10^((l_to - l_from) / 20), computed in float64 and rounded once to float32."""
    return np.float32(10.0 ** (gain_db(l_from, l_to) / 20.0))


def match_loudness(signal, l_from: float, l_to: float):
    """signal (float32 tensor or array) times gain_factor(l_from, l_to): ONE float32 multiply per sample."""
    g = gain_factor(l_from, l_to)
    if not math.isfinite(float(g)):
        raise ValueError(f"match_loudness: no finite gain from {l_from} to {l_to} LUFS")
    if isinstance(signal, torch.Tensor):
        if signal.dtype != torch.float32:
            raise TypeError(f"match_loudness: float32 samples (got {signal.dtype})")
        return signal * float(g)
    return _samples(signal).reshape(np.shape(signal)) * g


def check_rate(sr: int) -> None:
    """ValueError for a rate the resampler in front of the measure does not take."""
    sr = int(sr)
    if sr < 1:
        raise ValueError(f"loudness: the rate must be positive (got {sr})")
    if sr != SR and not fd_resample.bank_fits(sr, SR, RESAMPLE_WIDTH):
        raise ValueError(f"loudness: the filter bank of {sr} -> {SR} Hz is over the resampler's cap; the measure is defined at {SR} Hz "
                         f"(resample the signal yourself)")


def integrated_loudness(x, sr: int = SR) -> float:
    """The yardstick: x float32 [n] at rate sr -> LUFS (NaN for fewer than 19200 samples at 48 kHz, -inf for silence)."""
    check_rate(sr)
    x = _samples(x)
    if int(sr) != SR:
        x = audio.resample(torch.from_numpy(np.ascontiguousarray(x)), int(sr), SR, lowpass_filter_width=RESAMPLE_WIDTH).numpy()
    return lufs_of(gate(kweight_energies(x))[0])


def host_loudness(signals, sr: int = SR, batch: int = 8) -> np.ndarray:
    """integrated_loudness of every signal -> float64 [n] (the Scorer function of eval_cli.HOST_SCORER)."""
    return np.array([integrated_loudness(s, sr) for s in signals], np.float64)


# ---- loudness range (EBU Tech 3342), true peak (BS.1770 Annex 2) and the output gain of EBU R 128: the yardsticks ----------------------------
# Loudness range, on the sub-block energies E of step 3 above (`range_of`; every operation one float64 operation, as everywhere here):
#   a. Fewer than SHORT_SUBS = 30 sub-blocks: NaN, counts (0, 0, 0).  st_j = (((E[j] + E[j+1]) + ...) + E[j+29]) / 144000 for j = 0 ..
#      J - 30: a short-term (3 s) window starts at every sub-block -- a hop of 100 ms, 96.7 % overlap, inside Tech 3342's minimum.
#   b. A window that is NaN or Inf: NaN, counts (windows, 0, 0).
#   c. keep1 = st > ABS_GATE; n1 = 0: st_lo = st_hi = 0.0, and the range is 0.0 LU by definition (`lra_of`).
#   d. thr = 0.01 * (_lane_sum(st, keep1) / n1) (-20 LU on the mean square); keep2 = keep1 & (st > thr), m = n2 >= 1.
#   e. With s the kept values in ascending order: st_lo = s[((m - 1) * 10 + 50) // 100], st_hi = s[((m - 1) * 95 + 50) // 100] (the 10th
#      and the 95th percentile by nearest rank, in integer arithmetic).  Selection by value: ties cannot matter.
#   f. LRA = 10 log10(st_hi) - 10 log10(st_lo) is formed here, in Python, also from the device's values.  No logarithm decides a comparison.
# True peak (`true_peak_lin`): with H = align.frac_bank(4, W), a 4x oversampling interpolator,
#       p = max over n in [lo, hi), j in 0..3 of | sum_{t = 0 .. 2W-1} f64(x[n + t - W + 1]) * H[j][t] |
#   t ascending, every product and every sum rounded to float64 on its own, samples outside [0, len) zero, no rounding to float32.  Row 0
#   of the bank is the unit impulse: the sample peak is included.  A NaN or Inf sample among those the window reads (x[lo - W + 1 .. hi + W
#   - 1]) gives NaN -- every position that reads it has a sum that is not finite --, an empty clip NaN, an empty window of a clip that is
#   not empty 0.0 (the maximum of no magnitudes).  dBTP = 20 log10(p) is formed in Python (`dbtp_of`).
#   The interpolator is the project's own Hann-windowed sinc with TP_W = 12 (24 taps per phase), NOT the example filter of BS.1770-4 Annex
#   2 (12 taps per phase; its coefficients are not restated here).  On faded tones it reads within 0.005 dB of the analytic peak
#   (tests/test_loudness_range_cpu.py); a signal that starts or ends abruptly rings against the zeros around it, which is the definition.
TP_Q = 4
TP_W = 12
REL_GATE_RANGE = 0.01                       # -20 LU, on the mean square
SHORT_SAMPLES = SHORT_SUBS * SUB            # 144000
LRA_LO, LRA_HI = 10, 95                     # the percentiles of Tech 3342


def short_term_mean_squares(E) -> np.ndarray:
    """E [J] -> st [max(J - 29, 0)]: (((E[j] + E[j+1]) + ...) + E[j+29]) / 144000."""
    E = np.asarray(E, np.float64).reshape(-1)
    n = E.shape[0] - SHORT_SUBS + 1
    if n <= 0:
        return np.zeros(0, np.float64)
    with np.errstate(all="ignore"):
        a = E[0:n] + E[1:n + 1]
        for k in range(2, SHORT_SUBS):
            a = a + E[k:n + k]
        return a / float(SHORT_SAMPLES)


def range_ranks(m: int):
    """-> (i_lo, i_hi): the nearest ranks of the 10th and the 95th percentile among m >= 1 sorted values."""
    return ((m - 1) * LRA_LO + 50) // 100, ((m - 1) * LRA_HI + 50) // 100


def range_of(E):
    """E float64 [J] -> (st_lo, st_hi float64, counts int32 [3] = windows, windows above the absolute gate, windows above both): steps a to
    e above."""
    st = short_term_mean_squares(E)
    nwin = st.shape[0]
    nan = np.float64(np.nan)
    if nwin == 0:
        return nan, nan, np.zeros(3, np.int32)
    if not np.all(np.isfinite(st)):
        return nan, nan, np.array([nwin, 0, 0], np.int32)
    keep1 = st > ABS_GATE
    n1 = int(np.count_nonzero(keep1))
    if n1 == 0:
        return np.float64(0.0), np.float64(0.0), np.array([nwin, 0, 0], np.int32)
    thr = np.float64(REL_GATE_RANGE) * (_lane_sum(st, keep1) / np.float64(n1))
    keep2 = keep1 & (st > thr)
    m = int(np.count_nonzero(keep2))
    s = np.sort(st[keep2])
    i_lo, i_hi = range_ranks(m)
    return s[i_lo], s[i_hi], np.array([nwin, n1, m], np.int32)


def lra_of(st_lo, st_hi):
    """10 log10(st_hi) - 10 log10(st_lo): two mean squares (scalars or arrays) -> LU; 0.0 where both are 0 (nothing above the absolute
    gate), NaN -> NaN."""
    lo, hi = np.asarray(st_lo, np.float64), np.asarray(st_hi, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        out = np.where((lo == 0.0) & (hi == 0.0), 0.0, 10.0 * np.log10(hi) - 10.0 * np.log10(lo))
    return float(out) if out.ndim == 0 else out


def _at_48k(x, sr: int) -> np.ndarray:
    check_rate(sr)
    x = _samples(x)
    if int(sr) != SR:
        x = audio.resample(torch.from_numpy(np.ascontiguousarray(x)), int(sr), SR, lowpass_filter_width=RESAMPLE_WIDTH).numpy()
    return x


def loudness_range(x, sr: int = SR, return_counts: bool = False):
    """The yardstick: x float32 [n] at rate sr -> LU (NaN for fewer than 144000 samples at 48 kHz, 0.0 for silence)."""
    st_lo, st_hi, counts = range_of(kweight_energies(_at_48k(x, sr)))
    return (lra_of(st_lo, st_hi), counts) if return_counts else lra_of(st_lo, st_hi)


def host_loudness_range(signals, sr: int = SR, batch: int = 8) -> np.ndarray:
    """loudness_range of every signal -> float64 [n] (a Scorer function of eval_cli.HOST_SCORER)."""
    return np.array([loudness_range(s, sr) for s in signals], np.float64)


def _tp_width(W) -> int:
    W = int(W)
    if not 1 <= W <= align.MAX_W:
        raise ValueError(f"true peak: W must be in [1, {align.MAX_W}] (got {W})")
    return W


def true_peak_lin(x, lo: int = 0, hi=None, W: int = TP_W) -> np.float64:
    """x float32 [n] at 48 kHz -> p float64 of the definition above over the positions [lo, hi) (clamped into [0, n]; default: all)."""
    W = _tp_width(W)
    x = _samples(x)
    n = x.shape[0]
    if n == 0:
        return np.float64(np.nan)
    lo = min(max(int(lo), 0), n)
    hi = min(max(n if hi is None else int(hi), lo), n)
    if hi == lo:
        return np.float64(0.0)
    if not np.all(np.isfinite(x[max(lo - W + 1, 0):min(hi + W, n)])):
        return np.float64(np.nan)
    H = align.frac_bank(TP_Q, W)
    s0 = max(lo - W + 1, 0)
    xp = np.concatenate([np.zeros(W - 1, np.float64), x[s0:min(hi + W, n)].astype(np.float64), np.zeros(W, np.float64)])
    first = lo - s0                                      # xp[first + i + t] = x[lo + i + t - W + 1], zeros outside [0, n)
    cnt = hi - lo
    p = np.float64(0.0)
    for j in range(TP_Q):
        acc = np.zeros(cnt, np.float64)
        for t in range(2 * W):
            acc = acc + xp[first + t:first + t + cnt] * H[j, t]
        p = max(p, np.float64(np.max(np.abs(acc))))
    return p


def dbtp_of(p):
    """20 log10(p): a linear true peak (scalar or array) -> dBTP; 0 -> -inf, NaN -> NaN."""
    with np.errstate(divide="ignore", invalid="ignore"):
        out = 20.0 * np.log10(np.asarray(p, np.float64))
    return float(out) if out.ndim == 0 else out


def true_peak(x, sr: int = SR, W: int = TP_W) -> float:
    """The yardstick: x float32 [n] at rate sr -> dBTP (NaN for an empty clip or a NaN / Inf sample, -inf for silence)."""
    return dbtp_of(true_peak_lin(_at_48k(x, sr), W=W))


def host_true_peak(signals, sr: int = SR, batch: int = 8) -> np.ndarray:
    """true_peak of every signal -> float64 [n] (a Scorer function of eval_cli.HOST_SCORER)."""
    return np.array([true_peak(s, sr) for s in signals], np.float64)


def output_gain(lufs: float, dbtp: float, target_lufs: float, ceiling_dbtp=None):
    """-> (gain_db, limited): the gain that brings a signal of `lufs` to `target_lufs`, capped so that its true peak `dbtp` stays at or
    under `ceiling_dbtp` (a gain CAP, not a limiter: the signal is only scaled).  A lufs or dbtp that is not finite: (None, False) -- no
    gain, and the caller leaves the signal as it is."""
    lufs, dbtp = float(lufs), float(dbtp)
    if not (math.isfinite(lufs) and math.isfinite(dbtp)):
        return None, False
    g, limited = float(target_lufs) - lufs, False
    if ceiling_dbtp is not None and dbtp + g > float(ceiling_dbtp):
        g, limited = float(ceiling_dbtp) - dbtp, True
    return g, limited


def normalize_loudness(signal, lufs: float, dbtp: float, target_lufs: float, ceiling_dbtp=None):
    """-> (signal times the float32 factor of output_gain's gain -- ONE float32 multiply per sample, `match_loudness`'s rule --, gain_db,
    limited).  No gain (output_gain): the signal itself, None, False."""
    g, limited = output_gain(lufs, dbtp, target_lufs, ceiling_dbtp)
    if g is None:
        return signal, None, False
    return match_loudness(signal, 0.0, g), g, limited


def file_energies(channel_energies) -> np.ndarray:
    """The energies of a file of several channels: E_file[j] = E_0[j] + E_1[j] + ... with the channels ascending (BS.1770 with unit
    channel weights); `gate` then gates the file once."""
    Es = [np.asarray(E, np.float64).reshape(-1) for E in channel_energies]
    if not Es:
        raise ValueError("file_energies: no channel")
    out = Es[0].copy()
    with np.errstate(all="ignore"):
        for E in Es[1:]:
            if E.shape != out.shape:
                raise ValueError("file_energies: the channels of a file are equally long")
            out = out + E
    return out


def file_level(channels, sr: int = SR):
    """channels: the float32 [n] channels of ONE file -> (lufs, dbtp) of the file: the channel energies added (`file_energies`) and gated
    once, the true peak the maximum over the channels (NaN if any is NaN)."""
    chans = [_at_48k(c, sr) for c in channels]
    lufs = lufs_of(gate(file_energies([kweight_energies(c) for c in chans]))[0])
    peaks = [true_peak_lin(c) for c in chans]
    p = np.float64(np.nan) if any(np.isnan(q) for q in peaks) else max(peaks)
    return lufs, dbtp_of(p)


# ---- the same measure on the GPU (csrc/loudness.hip) -------------------------------------------------------------------------------------
def device_tables():
    """(M_CHUNK, M_SUB, ABS_GATE) as the library holds them (fd_loudness_tables; no GPU needed)."""
    mc, ms, g = np.zeros(16, np.float64), np.zeros(16, np.float64), C.c_double()
    L.check(L.load().fd_loudness_tables(mc.ctypes.data_as(C.c_void_p), ms.ctypes.data_as(C.c_void_p), C.byref(g)))
    return mc.reshape(4, 4), ms.reshape(4, 4), float(g.value)


def _workspace(lib, B, Lrow, device):
    nws = lib.fd_loudness_workspace_bytes(B, Lrow)
    if nws == 0:
        raise ValueError(f"loudness: no workspace for B {B}, L {Lrow}")
    return torch.empty(nws, dtype=torch.uint8, device=device), nws


def _device_clips(signals, sr, device):
    check_rate(sr)
    clips = []
    for i, c in enumerate(signals):
        c = torch.as_tensor(c).reshape(-1)
        if c.dtype != torch.float32:
            raise TypeError(f"loudness: float32 samples (clip {i} is {c.dtype})")
        if int(sr) != SR and c.numel():
            c = fd_resample.resample_device(c.to(device), int(sr), SR, lowpass_filter_width=RESAMPLE_WIDTH)
        clips.append(c)
    return clips


@torch.no_grad()
def energies_batch(signals, sr: int = SR, batch: int = 8, device="cuda"):
    """kweight_energies of every signal on the GPU (fd_loudness_energies, zero state) -> a list of float64 arrays [n_b // 4800]."""
    lib = L.load()
    clips = _device_clips(signals, sr, device)
    out = [np.zeros(0, np.float64) for _ in clips]
    idx = [i for i, c in enumerate(clips) if c.numel() >= SUB]
    got = np.empty(len(idx), object)

    def call(rows, lens, sel, Lmax):
        B = len(sel)
        ws, nws = _workspace(lib, B, Lmax, device)
        E = torch.empty(B, Lmax // SUB, dtype=torch.float64, device=device)
        nsub = torch.empty(B, dtype=torch.int32, device=device)
        L.check(lib.fd_loudness_energies(L.ptr(rows[0]), L.ptr(lens), B, Lmax, None, L.ptr(E), L.ptr(nsub), L.ptr(ws), nws, L.stream()))
        E, nsub = E.cpu().numpy(), nsub.cpu().numpy()
        res = np.empty(B, object)
        for b in range(B):
            res[b] = E[b, :nsub[b]].copy()
        return [res]

    if idx:
        ragged_batches(([clips[i] for i in idx],), batch, device, call, [got])
    for k, i in enumerate(idx):
        out[i] = got[k]
    return out


@torch.no_grad()
def loudness_ms_batch(signals, sr: int = SR, batch: int = 8, device="cuda"):
    """(ms_gated float64 [n], counts int32 [n, 3]) of every signal on the GPU: fd_loudness over length-sorted ragged batches of `batch`
    clips.  A clip's bits do not depend on the batch it ran in.  An empty clip is NaN with counts 0 without a call."""
    lib = L.load()
    clips = _device_clips(signals, sr, device)
    ms = np.full(len(clips), np.nan, np.float64)
    counts = np.zeros((len(clips), 3), np.int32)
    idx = [i for i, c in enumerate(clips) if c.numel() > 0]
    got_ms, got_counts = np.zeros(len(idx), np.float64), np.zeros((len(idx), 3), np.int32)

    def call(rows, lens, sel, Lmax):
        B = len(sel)
        ws, nws = _workspace(lib, B, Lmax, device)
        m = torch.empty(B, dtype=torch.float64, device=device)
        c = torch.empty(B, 3, dtype=torch.int32, device=device)
        L.check(lib.fd_loudness(L.ptr(rows[0]), L.ptr(lens), B, Lmax, L.ptr(m), L.ptr(c), L.ptr(ws), nws, L.stream()))
        return [m.cpu().numpy(), c.cpu().numpy()]

    if idx:
        ragged_batches(([clips[i] for i in idx],), batch, device, call, [got_ms, got_counts])
        ms[idx], counts[idx] = got_ms, got_counts
    return ms, counts


def loudness_batch(signals, sr: int = SR, batch: int = 8, device="cuda", return_counts: bool = False):
    """Integrated loudness of every signal (1-D float32, any lengths, at rate sr) on the GPU -> LUFS float64 [n] (return_counts: and
    int32 [n, 3] = blocks, above the absolute gate, above both).  NaN for a clip under 400 ms or with a NaN / Inf sample, -inf for
    silence."""
    ms, counts = loudness_ms_batch(signals, sr, batch, device)
    return (lufs_of(ms), counts) if return_counts else lufs_of(ms)


def _tp_taps(W: int, device) -> torch.Tensor:
    """align.frac_bank(4, W) on the device, float64 [4, 2 W]: one tensor per (device, W)."""
    dev = L.cuda_device(device)
    return L.cached_plan(dev, ("true_peak_taps", int(W)), lambda: torch.from_numpy(np.array(align.frac_bank(TP_Q, W))).to(dev))      # (a copy: the bank is read-only)


def _true_peak_rows(lib, rows, lens, B, Lrow, device, lo=None, hi=None, W: int = TP_W) -> torch.Tensor:
    """fd_true_peak on staged rows -> p DEVICE float64 [B]; lo, hi: int32 [B] on the device, or None for every position."""
    nws = lib.fd_true_peak_workspace_bytes(B, Lrow)
    if nws == 0:
        raise ValueError(f"true peak: no workspace for B {B}, L {Lrow}")
    ws = torch.empty(nws, dtype=torch.uint8, device=device)
    p = torch.empty(B, dtype=torch.float64, device=device)
    L.check(lib.fd_true_peak(L.ptr(rows), L.ptr(lens), B, Lrow, L.ptr(lo), L.ptr(hi), L.ptr(_tp_taps(W, device)), int(W), L.ptr(p), L.ptr(ws), nws,
                             L.stream()))
    return p


def _range_rows(lib, E, nsub, B, J, device):
    """fd_loudness_range on E DEVICE float64 [B, J] (None for J = 0), nsub DEVICE int32 [B] -> (st DEVICE float64 [B, 2], counts DEVICE
    int32 [B, 3])."""
    nws = lib.fd_loudness_range_workspace_bytes(B, J)
    if nws == 0:
        raise ValueError(f"loudness range: no workspace for B {B}, J {J}")
    ws = torch.empty(nws, dtype=torch.uint8, device=device)
    st = torch.empty(B, 2, dtype=torch.float64, device=device)
    counts = torch.empty(B, 3, dtype=torch.int32, device=device)
    L.check(lib.fd_loudness_range(L.ptr(E) if J else None, L.ptr(nsub), B, J, L.ptr(st), L.ptr(counts), L.ptr(ws), nws, L.stream()))
    return st, counts


def _energies_rows(lib, rows, lens, B, Lmax, device):
    """fd_loudness_energies (zero state) on staged rows -> (E DEVICE float64 [B, Lmax // 4800], nsub DEVICE int32 [B])."""
    ws, nws = _workspace(lib, B, Lmax, device)
    E = torch.empty(B, Lmax // SUB, dtype=torch.float64, device=device)
    nsub = torch.empty(B, dtype=torch.int32, device=device)
    L.check(lib.fd_loudness_energies(L.ptr(rows), L.ptr(lens), B, Lmax, None, L.ptr(E) if Lmax >= SUB else None, L.ptr(nsub), L.ptr(ws), nws,
                                     L.stream()))
    return E, nsub


@torch.no_grad()
def true_peak_lin_batch(signals, sr: int = SR, batch: int = 8, device="cuda", W: int = TP_W) -> np.ndarray:
    """true_peak_lin of every signal on the GPU (fd_true_peak over length-sorted ragged batches) -> p float64 [n].  A clip's bits do not
    depend on the batch it ran in.  An empty clip is NaN without a call."""
    W = _tp_width(W)
    lib = L.load()
    clips = _device_clips(signals, sr, device)
    p = np.full(len(clips), np.nan, np.float64)
    idx = [i for i, c in enumerate(clips) if c.numel() > 0]
    got = np.zeros(len(idx), np.float64)

    def call(rows, lens, sel, Lmax):
        return [_true_peak_rows(lib, rows[0], lens, len(sel), Lmax, device, W=W).cpu().numpy()]

    if idx:
        ragged_batches(([clips[i] for i in idx],), batch, device, call, [got])
        p[idx] = got
    return p


def true_peak_batch(signals, sr: int = SR, batch: int = 8, device="cuda") -> np.ndarray:
    """True peak of every signal (1-D float32, any lengths, at rate sr) on the GPU -> dBTP float64 [n]: NaN for an empty clip or one
    with a NaN / Inf sample, -inf for silence."""
    return dbtp_of(true_peak_lin_batch(signals, sr, batch, device))


@torch.no_grad()
def loudness_report_batch(signals, sr: int = SR, batch: int = 8, device="cuda", return_counts: bool = False, parts=("lufs", "lra", "dbtp")) -> dict:
    """Integrated loudness, loudness range and true peak of every signal from ONE staging of the clips -> {"lufs": LUFS float64 [n],
    "lra": LU float64 [n], "dbtp": dBTP float64 [n]} (return_counts: also "lufs_counts" and "lra_counts", int32 [n, 3]).  Each is, bit for
    bit, what loudness_batch, loudness_range_batch and true_peak_batch give: the energies of fd_loudness_energies go to fd_loudness_gate
    and to fd_loudness_range, the staged rows to fd_true_peak.  parts: the measures to take (the others are left out of the result)."""
    lib = L.load()
    clips = _device_clips(signals, sr, device)
    n = len(clips)
    nan = lambda: np.full(n, np.nan, np.float64)                      # noqa: E731
    ms, st_lo, st_hi, p = nan(), nan(), nan(), nan()
    c_gate, c_range = np.zeros((n, 3), np.int32), np.zeros((n, 3), np.int32)
    idx = [i for i, c in enumerate(clips) if c.numel() > 0]
    k = len(idx)
    got = [np.zeros(k, np.float64), np.zeros((k, 3), np.int32), np.zeros((k, 2), np.float64), np.zeros((k, 3), np.int32), np.zeros(k, np.float64)]
    want_e = "lufs" in parts or "lra" in parts

    def call(rows, lens, sel, Lmax):
        B, J = len(sel), Lmax // SUB
        out = [np.full(B, np.nan), np.zeros((B, 3), np.int32), np.full((B, 2), np.nan), np.zeros((B, 3), np.int32), np.full(B, np.nan)]
        if want_e:
            E, nsub = _energies_rows(lib, rows[0], lens, B, Lmax, device)
        if "lufs" in parts:
            m = torch.empty(B, dtype=torch.float64, device=device)
            c = torch.empty(B, 3, dtype=torch.int32, device=device)
            L.check(lib.fd_loudness_gate(L.ptr(E) if J else None, L.ptr(nsub), B, J, L.ptr(m), L.ptr(c), L.stream()))
            out[0], out[1] = m.cpu().numpy(), c.cpu().numpy()
        if "lra" in parts:
            st, c = _range_rows(lib, E, nsub, B, J, device)
            out[2], out[3] = st.cpu().numpy(), c.cpu().numpy()
        if "dbtp" in parts:
            out[4] = _true_peak_rows(lib, rows[0], lens, B, Lmax, device).cpu().numpy()
        return out

    if idx:
        ragged_batches(([clips[i] for i in idx],), batch, device, call, got)
        ms[idx], c_gate[idx], st_lo[idx], st_hi[idx], c_range[idx], p[idx] = got[0], got[1], got[2][:, 0], got[2][:, 1], got[3], got[4]
    res = {}
    if "lufs" in parts:
        res["lufs"] = lufs_of(ms)
    if "lra" in parts:
        res["lra"] = lra_of(st_lo, st_hi)
    if "dbtp" in parts:
        res["dbtp"] = dbtp_of(p)
    if return_counts:
        if "lufs" in parts:
            res["lufs_counts"] = c_gate
        if "lra" in parts:
            res["lra_counts"] = c_range
    return res


def loudness_range_batch(signals, sr: int = SR, batch: int = 8, device="cuda", return_counts: bool = False):
    """Loudness range of every signal (1-D float32, any lengths, at rate sr) on the GPU -> LU float64 [n] (return_counts: and int32
    [n, 3] = short-term windows, above the absolute gate, above both).  NaN for a clip under 3 s or with a NaN / Inf sample, 0.0 for
    silence."""
    res = loudness_report_batch(signals, sr, batch, device, return_counts=True, parts=("lra",))
    return (res["lra"], res["lra_counts"]) if return_counts else res["lra"]


@torch.no_grad()
def file_level_batch(files, sr: int = SR, batch: int = 8, device="cuda", peak: bool = True):
    """files: one list of channels (1-D float32, equally long) per file -> (lufs float64 [n], dbtp float64 [n]) of the FILES: the channel
    energies of fd_loudness_energies added with the channels ascending (`file_energies`) and gated once (`gate`), the true peak the
    maximum over the channels (NaN if any is NaN).  A file of one channel reads what loudness_batch and true_peak_batch give.  The
    channels are staged ONCE: fd_loudness_energies and fd_true_peak read the same rows.  peak=False: no true peak is taken (dbtp NaN)."""
    lib = L.load()
    clips = _device_clips([c for chans in files for c in chans], sr, device)
    Es = [np.zeros(0, np.float64) for _ in clips]
    ps = np.full(len(clips), np.nan, np.float64)
    idx = [i for i, c in enumerate(clips) if c.numel() > 0]
    got_E, got_p = np.empty(len(idx), object), np.full(len(idx), np.nan, np.float64)

    def call(rows, lens, sel, Lmax):
        B = len(sel)
        E, nsub = _energies_rows(lib, rows[0], lens, B, Lmax, device)
        p = _true_peak_rows(lib, rows[0], lens, B, Lmax, device).cpu().numpy() if peak else np.full(B, np.nan)
        E, nsub = E.cpu().numpy(), nsub.cpu().numpy()
        res = np.empty(B, object)
        for b in range(B):
            res[b] = E[b, :nsub[b]].copy()
        return [res, p]

    if idx:
        ragged_batches(([clips[i] for i in idx],), batch, device, call, [got_E, got_p])
    for k, i in enumerate(idx):
        Es[i], ps[i] = got_E[k], got_p[k]
    lufs, dbtp, k = np.zeros(len(files), np.float64), np.zeros(len(files), np.float64), 0
    for i, chans in enumerate(files):
        nc = len(chans)
        lufs[i] = lufs_of(gate(file_energies(Es[k:k + nc]))[0])
        dbtp[i] = dbtp_of(np.nan if np.any(np.isnan(ps[k:k + nc])) else np.max(ps[k:k + nc]))
        k += nc
    return lufs, dbtp


class LoudnessMeter:
    """A streaming meter at 48 kHz: `push(block)` takes float32 or int16 PCM (x * 2^-15, exact) of any size, tensors or arrays, on the
    CPU or the device.  The samples that do not yet fill a sub-block (at most 4799) are held back; the whole sub-blocks are filtered from
    the carried state (fd_loudness_energies) and their energies kept on the device.  `integrated()` (fd_loudness_gate over everything so
    far), `momentary()` (the last 4 sub-blocks) and `short_term()` (the last 30) are what the one-shot call gives on the concatenated
    input, bit for bit, however it was cut into pushes.  So are `loudness_range()` (fd_loudness_range over the energies so far) and
    `true_peak()`: a position's 2 W taps read W samples behind it, so every push commits the maximum over the positions whose taps have
    all arrived and keeps the last 2 W - 1 samples; `true_peak()` answers with the maximum of that and of the uncommitted tail read with
    zeros behind it -- both through fd_true_peak's window, and without touching the meter's state.  Another rate: put a
    `resample.ResampleStream` in front."""

    def __init__(self, device="cuda"):
        self.dev = L.cuda_device(device)
        if self.dev.type != "cuda":
            raise RuntimeError("flowdec_amd: LoudnessMeter runs on the GPU (HIP is the only compute path)")
        self._state = torch.zeros(1, 4, dtype=torch.float64, device=self.dev)
        self._pending = torch.empty(0, dtype=torch.float32, device=self.dev)
        self._E = torch.empty(0, dtype=torch.float64, device=self.dev)
        self.received = 0
        self._tp_tail = torch.empty(0, dtype=torch.float32, device=self.dev)    # the samples from max(_tp_done - W + 1, 0) on
        self._tp_done = 0                                                       # positions committed: max(received - W, 0)
        self._tp_commit = torch.zeros(1, dtype=torch.float64, device=self.dev)  # their maximum (NaN once a sum was not finite)

    def _peak_window(self, buf: torch.Tensor, lo: int, hi: int) -> torch.Tensor:
        """fd_true_peak over the positions [lo, hi) of the one row buf -> p DEVICE float64 [1]."""
        n = int(buf.numel())
        meta = torch.tensor([n, lo, hi], dtype=torch.int32).to(self.dev)
        with torch.cuda.device(self.dev):
            return _true_peak_rows(L.load(), buf.reshape(1, -1), meta[0:1], 1, n, self.dev, lo=meta[1:2], hi=meta[2:3])

    def _push_peak(self, x: torch.Tensor) -> None:
        first = max(self._tp_done - TP_W + 1, 0)                  # the sample index of buf[0]
        buf = torch.cat([self._tp_tail, x]) if self._tp_tail.numel() else x
        done = max(self.received - TP_W, 0)
        if done > self._tp_done:
            self._tp_commit = torch.maximum(self._tp_commit, self._peak_window(buf.contiguous(), self._tp_done - first, done - first))
            self._tp_done = done
        self._tp_tail = buf[max(done - TP_W + 1, 0) - first:].clone()

    def _block(self, x) -> torch.Tensor:
        x = torch.as_tensor(x).reshape(-1)
        if x.is_cuda and x.device != self.dev:
            raise RuntimeError(f"LoudnessMeter.push: the block lives on {x.device}, the meter on {self.dev}")
        if x.dtype == torch.int16:
            return x.to(self.dev).to(torch.float32) * (1.0 / 32768.0)
        if x.dtype != torch.float32:
            raise TypeError(f"LoudnessMeter.push: float32 or int16 samples (got {x.dtype})")
        return x.to(self.dev)

    @torch.no_grad()
    def push(self, x) -> int:
        """-> the number of sub-blocks this push completed."""
        x = self._block(x)
        self.received += int(x.numel())
        if x.numel():
            self._push_peak(x)
        buf = torch.cat([self._pending, x]) if self._pending.numel() else x
        k = int(buf.numel()) // SUB
        if k:
            lib = L.load()
            rows = buf[:k * SUB].reshape(1, -1).contiguous()
            E = torch.empty(1, k, dtype=torch.float64, device=self.dev)
            nsub = torch.empty(1, dtype=torch.int32, device=self.dev)
            lens = torch.tensor([k * SUB], dtype=torch.int32).to(self.dev)
            with torch.cuda.device(self.dev):
                ws, nws = _workspace(lib, 1, k * SUB, self.dev)
                L.check(lib.fd_loudness_energies(L.ptr(rows), L.ptr(lens), 1, k * SUB, L.ptr(self._state), L.ptr(E), L.ptr(nsub), L.ptr(ws), nws,
                                                 L.stream()))
            self._E = torch.cat([self._E, E[0]])
        self._pending = buf[k * SUB:].clone()
        return k

    def energies(self) -> np.ndarray:
        """The sub-block energies so far, float64 [received // 4800]."""
        return self._E.cpu().numpy()

    @torch.no_grad()
    def integrated(self, return_counts: bool = False):
        J = int(self._E.numel())
        ms = torch.empty(1, dtype=torch.float64, device=self.dev)
        counts = torch.empty(1, 3, dtype=torch.int32, device=self.dev)
        nsub = torch.tensor([J], dtype=torch.int32).to(self.dev)
        with torch.cuda.device(self.dev):
            L.check(L.load().fd_loudness_gate(L.ptr(self._E) if J else None, L.ptr(nsub), 1, J, L.ptr(ms), L.ptr(counts), L.stream()))
        out = lufs_of(ms.cpu().numpy()[0])
        return (out, counts.cpu().numpy()[0]) if return_counts else out

    @torch.no_grad()
    def loudness_range(self, return_counts: bool = False):
        """The loudness range (LU) of everything pushed so far: NaN under 3 s."""
        J = int(self._E.numel())
        nsub = torch.tensor([J], dtype=torch.int32).to(self.dev)
        with torch.cuda.device(self.dev):
            st, counts = _range_rows(L.load(), self._E.reshape(1, -1) if J else None, nsub, 1, J, self.dev)
        st = st.cpu().numpy()[0]
        out = lra_of(st[0], st[1])
        return (out, counts.cpu().numpy()[0]) if return_counts else out

    @torch.no_grad()
    def true_peak(self) -> float:
        """The true peak (dBTP) of everything pushed so far, the end of the input read against zeros: NaN before the first sample."""
        if self.received == 0:
            return float("nan")
        first = max(self._tp_done - TP_W + 1, 0)
        p = torch.maximum(self._tp_commit, self._peak_window(self._tp_tail, self._tp_done - first, self.received - first))
        return dbtp_of(p.cpu().numpy()[0])

    def momentary(self) -> float:
        return momentary_of(self._E[-BLOCK_SUBS:].cpu().numpy())

    def short_term(self) -> float:
        return short_term_of(self._E[-SHORT_SUBS:].cpu().numpy())
