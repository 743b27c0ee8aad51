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
"""
import ctypes as C
import math

import numpy as np
import torch

from . import _lib as L
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


class LoudnessMeter:
    """A streaming meter at 48 kHz: `push(block)` takes float32 or int16 PCM (x * 2^-15, exact) of any size, tensors or arrays, on the
    CPU or the device.  The samples that do not yet fill a sub-block (at most 4799) are held back; the whole sub-blocks are filtered from
    the carried state (fd_loudness_energies) and their energies kept on the device.  `integrated()` (fd_loudness_gate over everything so
    far), `momentary()` (the last 4 sub-blocks) and `short_term()` (the last 30) are what the one-shot call gives on the concatenated
    input, bit for bit, however it was cut into pushes.  Another rate: put a `resample.ResampleStream` in front."""

    def __init__(self, device="cuda"):
        self.dev = L.cuda_device(device)
        if self.dev.type != "cuda":
            raise RuntimeError("flowdec_amd: LoudnessMeter runs on the GPU (HIP is the only compute path)")
        self._state = torch.zeros(1, 4, dtype=torch.float64, device=self.dev)
        self._pending = torch.empty(0, dtype=torch.float32, device=self.dev)
        self._E = torch.empty(0, dtype=torch.float64, device=self.dev)
        self.received = 0

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

    def momentary(self) -> float:
        return momentary_of(self._E[-BLOCK_SUBS:].cpu().numpy())

    def short_term(self) -> float:
        return short_term_of(self._E[-SHORT_SUBS:].cpu().numpy())
