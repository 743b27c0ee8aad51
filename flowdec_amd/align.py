"""Alignment in time of the three signals of a triple before they are scored, and of the coded signal of a (clean, coded) pair before
estimate_cli and loss_cli read it: a bounded-lag cross-correlation, the lag of its peak -- in whole samples or on a grid of 1 / Q samples,
with or without polarity -- and the cut to the common support.  Host yardsticks in NumPy float64 and the GPU path over ragged batches
(csrc/xcorr.hip, csrc/fracshift.hip, include/flowdec_hip.h "Alignment in time"), which eval_cli, estimate_cli and loss_cli run for --align.

* xcorr           c[l + M] = sum_n a[n] b[n + l] for l in [-M, M], n over max(0, -l) <= n < min(La, Lb - l); an empty range is exactly 0.0.
                  The signals are float32, products and sums float64.  A peak at l > 0 means b is a delayed by l samples.
* pick_lag        the l with the largest c, NaN counting as -inf; among equal maxima the smallest |l|, and of -l and +l it is +l; all NaN
                  or all equal (two silent signals) gives 0
* common_support  n0 = max(0, -lag_h, -lag_y), n1 = min(Lx, Lh - lag_h, Ly - lag_y): the samples n of x for which x_hat[n + lag_h] and
                  y[n + lag_y] exist
* align_triple    the three views on that support: equal lengths, no copy, no zero fill

Sub-sample delays and polarity (eval_cli --align-frac / --align-polarity; the --align of estimate_cli and loss_cli):

* frac_bank       H float64 [Q][2 W]: row j holds the taps k = -W + 1 .. W (column k + W - 1) of a Hann-windowed sinc that reads a signal
                  j / Q samples later: H[j][k] = sinc(u) (1 + cos(pi u / W)) / 2, u = k - j / Q, 0 where |u| >= W; row 0 is the unit
                  impulse.  Built on the host; the device only reads it.
* refine_lag      (lag_q, sign) of a correlation: l0 = pick_lag(|c| with polarity, else c), sign = -1 when polarity and c[l0] < 0, then
                  the q in [-(Q - 1), Q - 1], |l0 + q / Q| <= M, with the largest r(q) = sum_k (sign c[l0 + floor(q / Q) + k]) H[q mod Q][k]
                  (k ascending, products and sums separately rounded float64, indices outside [-M, M] left out, NaN as -inf; ties to the
                  smallest |q|, then +q; all -inf gives 0).  lag_q = l0 Q + q: the lag is lag_q / Q samples.  r(0) = sign c[l0] exactly.
* frac_shift      out[n - n0] = f32(sign sum_k f64(s[n + base + k]) H[j][k]), base = floor(lag_q / Q), j = lag_q mod Q, n in [n0, n1):
                  the signal read lag_q / Q samples later; samples outside [0, len) are zeros; the same order and rounding
* support_frac    the n for which no tap reads such a zero: [W - 1 - base, len - W - base) when j != 0, [-base, len - base) when j = 0
* align_triple_frac / align_pair_frac: the signals on the intersection of their supports with [0, Lx).  A signal with j = 0 and sign = +1 is
                  cut as a view, as align_triple cuts it, so whole-sample delays give the very samples of the integer path.

What is left out: clock drift (a lag that changes along the file) and alignment inside enhance; a level difference is
undone by loudness.py (eval_cli --match-loudness).

Imports `_lib` and `batching` only (no command line).
"""
import contextlib
import functools
import sys

import numpy as np
import torch

from . import _lib as L
from .batching import ragged_batches

MAX_LAG_CAP = 1 << 20       # fd_xcorr_lags refuses a larger max_lag


def _signal(a) -> np.ndarray:
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    return np.asarray(a, dtype=np.float32).reshape(-1)


def _max_lag(max_lag) -> int:
    M = int(max_lag)
    if M < 1 or M > MAX_LAG_CAP:
        raise ValueError(f"align: max_lag must be in [1, {MAX_LAG_CAP}] (got {max_lag})")
    return M


def xcorr(a, b, max_lag) -> np.ndarray:
    """-> c float64 [2 M + 1] of the definition above: one slice and one np.dot per lag (the yardstick: not clever on purpose)."""
    M = _max_lag(max_lag)
    a, b = _signal(a).astype(np.float64), _signal(b).astype(np.float64)
    c = np.zeros(2 * M + 1, np.float64)
    for l in range(-M, M + 1):
        lo, hi = max(0, -l), min(len(a), len(b) - l)
        if hi > lo:
            c[l + M] = np.dot(a[lo:hi], b[lo + l:hi + l])
    return c


def pick_lag(c) -> int:
    """The lag of the peak of c [2 M + 1] by the rule above."""
    c = np.asarray(c, dtype=np.float64).reshape(-1)
    if len(c) < 1 or len(c) % 2 != 1:
        raise ValueError(f"align: a correlation has 2 M + 1 values (got {len(c)})")
    M = (len(c) - 1) // 2
    v = np.where(np.isnan(c), -np.inf, c)
    best = np.nonzero(v == v.max())[0] - M
    return int(min(best, key=lambda l: (abs(int(l)), -int(l))))


def best_lag(a, b, max_lag) -> int:
    return pick_lag(xcorr(a, b, max_lag))


def common_support(Lx: int, Lh: int, Ly: int, lag_h: int, lag_y: int):
    """-> (n0, n1): the samples of x that x_hat delayed by lag_h and y delayed by lag_y both cover; empty when n1 <= n0."""
    return max(0, -int(lag_h), -int(lag_y)), min(int(Lx), int(Lh) - int(lag_h), int(Ly) - int(lag_y))


def align_triple(x_hat, x, y, lag_h: int, lag_y: int):
    """-> (x_hat[n0 + lag_h : n1 + lag_h], x[n0 : n1], y[n0 + lag_y : n1 + lag_y]): slices of the last axis (views of a tensor or an
    array), all three empty when the common support is."""
    lag_h, lag_y = int(lag_h), int(lag_y)
    n0, n1 = common_support(x.shape[-1], x_hat.shape[-1], y.shape[-1], lag_h, lag_y)
    n1 = max(n1, n0)
    return x_hat[..., n0 + lag_h:n1 + lag_h], x[..., n0:n1], y[..., n0 + lag_y:n1 + lag_y]


def _pairs(as_, bs):
    as_, bs = ([torch.as_tensor(c).reshape(-1) for c in l] for l in (as_, bs))
    if len(as_) != len(bs):
        raise ValueError("align: the lists must have one entry per pair each")
    return as_, bs


def host_lags(as_, bs, max_lag, batch=None, device=None, return_xcorr: bool = False):
    """best_lag of every pair on the host -> int64 [n] (with return_xcorr also float64 [n, 2 M + 1]); batch and device are not used."""
    M = _max_lag(max_lag)
    as_, bs = _pairs(as_, bs)
    cs = np.zeros((len(as_), 2 * M + 1), np.float64)
    for i, (a, b) in enumerate(zip(as_, bs)):
        cs[i] = xcorr(a, b, M)
    lags = np.array([pick_lag(c) for c in cs], np.int64).reshape(-1)
    return (lags, cs) if return_xcorr else lags


def _xcorr_batches(as_, bs, M, batch, device, return_xcorr, outs, native):
    """What lags_batch and lags_batch_frac share: the pairs (`_pairs`) sorted by the longer signal's length and cut into batches of
    `batch`, each list staged as zero-padded rows of its own length (batching.ragged_batches, own_rows); native(rows of a and b, their
    lens, B, La, Lb, c, ws, nws) makes the entry point's call and returns its results, which land in `outs`.  -> the float64
    [n, 2 M + 1] correlations or None."""
    lib = L.load()
    cs = np.zeros((len(as_), 2 * M + 1), np.float64) if return_xcorr else None

    def call(rows, lens, idx, Lrow):
        B, (La, Lb) = len(idx), Lrow
        nws = lib.fd_xcorr_workspace_bytes(B, La, Lb, M)       # (fd_xcorr_frac_workspace_bytes is the same number)
        ws = torch.empty(nws, dtype=torch.uint8, device=device)
        c = torch.empty(B, 2 * M + 1, dtype=torch.float64, device=device) if return_xcorr else None
        got = native(L.ptr(rows[0]), L.ptr(rows[1]), L.ptr(lens[0]), L.ptr(lens[1]), B, La, Lb, L.ptr(c), L.ptr(ws), nws)
        return got + ([c.cpu().numpy()] if return_xcorr else [])

    ragged_batches((as_, bs), batch, device, call, outs + ([cs] if return_xcorr else []), own_rows=True)
    return cs


def lags_batch(as_, bs, max_lag, batch: int = 8, device="cuda", return_xcorr: bool = False):
    """best_lag of every (a, b) on the GPU: lists of 1-D signals of any lengths (the two of a pair may differ) -> int64 [n] (with
    return_xcorr also the float64 [n, 2 M + 1] correlations).  Sorted by the longer signal's length and cut into batches of `batch` pairs;
    each list is staged as zero-padded rows of its own length (batching.padded_rows); a pair's numbers do not depend on its batch."""
    lib = L.load()
    M = _max_lag(max_lag)
    as_, bs = _pairs(as_, bs)
    lags = np.zeros(len(as_), np.int64)

    def native(a, b, lens_a, lens_b, B, La, Lb, c, ws, nws):
        out = torch.empty(B, dtype=torch.int32, device=device)
        L.check(lib.fd_xcorr_lags(a, b, lens_a, lens_b, B, La, Lb, M, c, L.ptr(out), ws, nws, L.stream()))
        return [out.cpu().numpy()]

    cs = _xcorr_batches(as_, bs, M, batch, device, return_xcorr, [lags], native)
    return (lags, cs) if return_xcorr else lags


# ---- sub-sample delays and polarity: the yardsticks ----------------------------------------------------------------------------------------
FRAC_Q, FRAC_W = 64, 32     # the grid (steps per sample) and the half width of the interpolator (2 W taps) of the command lines' defaults
MAX_Q, MAX_W = 1024, 256    # fd_xcorr_lags_frac / fd_frac_shift refuse more


def _grid(Q, W):
    Q, W = int(Q), int(W)
    if not 2 <= Q <= MAX_Q or not 1 <= W <= MAX_W:
        raise ValueError(f"align: Q must be in [2, {MAX_Q}] and W in [1, {MAX_W}] (got Q {Q}, W {W})")
    return Q, W


@functools.lru_cache(maxsize=8)
def _bank(Q: int, W: int) -> np.ndarray:
    u = np.arange(-W + 1, W + 1, dtype=np.float64)[None, :] - np.arange(Q, dtype=np.float64)[:, None] / Q
    H = np.sinc(u) * (0.5 * (1.0 + np.cos(np.pi * u / W)))
    H[np.abs(u) >= W] = 0.0
    H[0] = 0.0
    H[0, W - 1] = 1.0           # row 0 is the unit impulse, set and not computed
    H.setflags(write=False)
    return H


def frac_bank(Q: int = FRAC_Q, W: int = FRAC_W) -> np.ndarray:
    """-> H float64 [Q][2 W] of the definition above (read-only; one array per (Q, W))."""
    return _bank(*_grid(Q, W))


def _correlation(c):
    c = np.asarray(c, dtype=np.float64).reshape(-1)
    if len(c) < 1 or len(c) % 2 != 1:
        raise ValueError(f"align: a correlation has 2 M + 1 values (got {len(c)})")
    return c, (len(c) - 1) // 2


def pick_polarity(c, polarity: bool = True):
    """-> (l0, sign): pick_lag of |c| and the sign of c there (polarity=False: pick_lag(c), +1)."""
    c, M = _correlation(c)
    l0 = pick_lag(np.abs(c) if polarity else c)
    return l0, (-1 if polarity and c[l0 + M] < 0 else 1)


def refine_lag(c, Q: int = FRAC_Q, W: int = FRAC_W, polarity: bool = False):
    """-> (lag_q, sign) of c [2 M + 1] by the rule above: plain Python floats, one product and one addition at a time."""
    Q, W = _grid(Q, W)
    c, M = _correlation(c)
    H = frac_bank(Q, W).tolist()
    l0, sign = pick_polarity(c, polarity)
    sc = (float(sign) * c).tolist()                      # exact
    best = None
    for q in range(-(Q - 1), Q):
        if abs(l0 * Q + q) > M * Q:
            continue
        base, j = divmod(q, Q)
        r = 0.0
        for t in range(2 * W):
            l = l0 + base + t - W + 1
            if -M <= l <= M:
                r = r + sc[l + M] * H[j][t]
        if r != r:
            r = -np.inf
        if best is None or r > best[0] or (r == best[0] and (abs(q), -q) < (abs(best[1]), -best[1])):
            best = (r, q)
    return l0 * Q + (best[1] if best is not None else 0), sign


def frac_shift(s, lag_q: int, sign: int, Q: int, W: int, n0: int, n1: int) -> np.ndarray:
    """-> float32 [max(n1 - n0, 0)] of the definition above: one NumPy product and one NumPy addition per tap, for all n at once."""
    Q, W = _grid(Q, W)
    s = _signal(s).astype(np.float64)
    base, j = divmod(int(lag_q), Q)
    h = frac_bank(Q, W)[j]
    n = np.arange(int(n0), max(int(n1), int(n0)), dtype=np.int64)
    acc = np.zeros(len(n), np.float64)
    for t in range(2 * W):
        m = n + (base + t - W + 1)
        inside = (m >= 0) & (m < len(s))
        v = np.zeros(len(n), np.float64)
        v[inside] = s[m[inside]]
        acc = acc + v * h[t]
    return ((-1.0 if sign < 0 else 1.0) * acc).astype(np.float32)


def support_frac(length: int, lag_q: int, Q: int, W: int):
    """-> (lo, hi): the n for which a signal of `length` samples read lag_q / Q samples later needs no sample outside itself."""
    base, j = divmod(int(lag_q), int(Q))
    return (-base, int(length) - base) if j == 0 else (int(W) - 1 - base, int(length) - int(W) - base)


def common_support_frac(Lx: int, lengths, lag_qs, Q: int, W: int):
    """-> (n0, n1): [0, Lx) cut by support_frac of every (length, lag_q); empty when n1 <= n0."""
    sup = [support_frac(n, l, Q, W) for n, l in zip(lengths, lag_qs)]
    return max([0] + [lo for lo, _ in sup]), min([int(Lx)] + [hi for _, hi in sup])


def host_shift(signals, lag_q, sign, windows, Q: int = FRAC_Q, W: int = FRAC_W, batch=None, device=None):
    """frac_shift of every signal over its window (n0, n1) on the host -> float32 tensors; batch and device are not used."""
    return [torch.from_numpy(frac_shift(s, int(l), int(g), Q, W, int(w[0]), int(w[1]))) for s, l, g, w in zip(signals, lag_q, sign, windows)]


def cut_frac(signals, lag_q, sign, windows, Q: int, W: int, shift=host_shift, batch: int = 8):
    """Every signal over its window (n0, n1), read lag_q / Q samples later and multiplied by sign.  A signal with lag_q % Q == 0 and sign
    +1 is the view s[..., n0 + base : n1 + base] and no kernel runs for it; all others go through ONE call of `shift` (host_shift or
    shift_batch) and come back as new float32 tensors (arrays for array input)."""
    out, todo = [None] * len(signals), []
    for i, (s, l, g, (n0, n1)) in enumerate(zip(signals, lag_q, sign, windows)):
        base, j = divmod(int(l), int(Q))
        n1 = max(int(n1), int(n0))
        if j == 0 and int(g) >= 0:
            out[i] = s[..., int(n0) + base:n1 + base]
        else:
            todo.append(i)
    if todo:
        got = shift([torch.as_tensor(signals[i]).reshape(-1) for i in todo], [int(lag_q[i]) for i in todo], [int(sign[i]) for i in todo],
                    [(int(windows[i][0]), max(int(windows[i][1]), int(windows[i][0]))) for i in todo], Q, W, batch)
        for i, g in zip(todo, got):
            out[i] = g if isinstance(signals[i], torch.Tensor) else g.numpy()
    return out


def align_triple_frac(x_hat, x, y, lag_q_h: int, lag_q_y: int, sign_h: int = 1, sign_y: int = 1, Q: int = FRAC_Q, W: int = FRAC_W, shift=host_shift,
                      batch: int = 8):
    """-> (x_hat, x, y) on the common support of x_hat read lag_q_h / Q and y read lag_q_y / Q samples later, equal lengths; x is a view,
    and so is a signal whose delay is a whole number of samples and whose sign is +1 (align_triple's cut)."""
    n0, n1 = common_support_frac(x.shape[-1], (x_hat.shape[-1], y.shape[-1]), (lag_q_h, lag_q_y), Q, W)
    n1 = max(n1, n0)
    h, yy = cut_frac([x_hat, y], [lag_q_h, lag_q_y], [sign_h, sign_y], [(n0, n1)] * 2, Q, W, shift, batch)
    return h, x[..., n0:n1], yy


def align_pair_frac(x, y, lag_q: int, sign: int = 1, Q: int = FRAC_Q, W: int = FRAC_W, shift=host_shift, batch: int = 8):
    """-> (x, y) on the common support of x and y read lag_q / Q samples later."""
    n0, n1 = common_support_frac(x.shape[-1], (y.shape[-1],), (lag_q,), Q, W)
    n1 = max(n1, n0)
    return x[..., n0:n1], cut_frac([y], [lag_q], [sign], [(n0, n1)], Q, W, shift, batch)[0]


def host_lags_frac(as_, bs, max_lag, Q: int = FRAC_Q, W: int = FRAC_W, polarity: bool = False, batch=None, device=None, return_xcorr: bool = False):
    """refine_lag of xcorr of every pair on the host -> (lag_q int64 [n], sign int32 [n]) (with return_xcorr also float64 [n, 2 M + 1])."""
    _, cs = host_lags(as_, bs, max_lag, return_xcorr=True)
    got = [refine_lag(c, Q, W, polarity) for c in cs]
    lag_q, sign = np.array([g[0] for g in got], np.int64).reshape(-1), np.array([g[1] for g in got], np.int32).reshape(-1)
    return (lag_q, sign, cs) if return_xcorr else (lag_q, sign)


# ---- sub-sample delays and polarity: the GPU path ------------------------------------------------------------------------------------------
def lags_batch_frac(as_, bs, max_lag, Q: int = FRAC_Q, W: int = FRAC_W, polarity: bool = False, batch: int = 8, device="cuda",
                    return_xcorr: bool = False):
    """refine_lag of every (a, b) on the GPU (fd_xcorr_lags_frac) -> (lag_q int64 [n], sign int32 [n]) (with return_xcorr also the float64
    [n, 2 M + 1] correlations): sorted, cut and staged like lags_batch; a pair's numbers do not depend on its batch."""
    lib = L.load()
    M = _max_lag(max_lag)
    Q, W = _grid(Q, W)
    as_, bs = _pairs(as_, bs)
    lag_q, sign = np.zeros(len(as_), np.int64), np.ones(len(as_), np.int32)
    bank = torch.tensor(frac_bank(Q, W)).to(device)

    def native(a, b, lens_a, lens_b, B, La, Lb, c, ws, nws):
        out_q = torch.empty(B, dtype=torch.int64, device=device)
        out_s = torch.empty(B, dtype=torch.int32, device=device)
        L.check(lib.fd_xcorr_lags_frac(a, b, lens_a, lens_b, B, La, Lb, M, L.ptr(bank), Q, W, int(bool(polarity)), c, L.ptr(out_q), L.ptr(out_s), ws, nws,
                                       L.stream()))
        return [out_q.cpu().numpy(), out_s.cpu().numpy()]

    cs = _xcorr_batches(as_, bs, M, batch, device, return_xcorr, [lag_q, sign], native)
    return (lag_q, sign, cs) if return_xcorr else (lag_q, sign)


def shift_batch(signals, lag_q, sign, windows, Q: int = FRAC_Q, W: int = FRAC_W, batch: int = 8, device="cuda"):
    """frac_shift of every signal over its window (n0, n1) on the GPU (fd_frac_shift) -> float32 tensors on the host, bit for bit the
    yardstick's.  Sorted by the signal's length and cut into batches of `batch`; staged through batching.ragged_batches."""
    lib = L.load()
    Q, W = _grid(Q, W)
    signals = [torch.as_tensor(s).reshape(-1) for s in signals]
    if not len(signals) == len(lag_q) == len(sign) == len(windows):
        raise ValueError("align: one lag, one sign and one window per signal")
    H = frac_bank(Q, W)
    split = [divmod(int(l), Q) for l in lag_q]
    win = [(int(a), max(int(b), int(a))) for a, b in windows]
    if any(abs(v) >= 1 << 31 for bj, w in zip(split, win) for v in (bj[0], w[0], w[1])):
        raise ValueError("align: a lag or a window beyond 32 bits")
    out = [None] * len(signals)

    def call(rows, lens, idx, Lrow):
        B, Ls, Lo = len(idx), Lrow[0], max(max(win[i][1] - win[i][0] for i in idx), 1)
        ints = torch.tensor([[split[i][0], int(sign[i]), win[i][0], win[i][1]] for i in idx], dtype=torch.int32).t().contiguous().to(device)
        taps = torch.from_numpy(np.stack([H[split[i][1]] for i in idx])).to(device)
        res = torch.empty(B, Lo, dtype=torch.float32, device=device)
        L.check(lib.fd_frac_shift(L.ptr(rows[0]), L.ptr(lens[0]), B, Ls, L.ptr(ints[0]), L.ptr(taps), W, L.ptr(ints[1]), L.ptr(ints[2]), L.ptr(ints[3]),
                                  L.ptr(res), Lo, L.stream()))
        res = res.cpu()
        return [[res[k, :win[i][1] - win[i][0]].clone() for k, i in enumerate(idx)]]

    ragged_batches((signals,), batch, device, call, [out], own_rows=True)     # (own_rows: a signal may be empty)
    return out


# ---- what the command lines share ----------------------------------------------------------------------------------------------------------
def find_lags(as_, bs, max_lag, frac: bool, polarity: bool, Q: int, W: int, batch: int, lags=lags_batch, lags_frac=lags_batch_frac):
    """-> (lag_q int64 [n], sign int32 [n]) of every b against its a, in units of 1 / Q sample.  frac: `lags_frac` (lags_batch_frac /
    host_lags_frac).  Else whole samples by `lags` (lags_batch / host_lags): lag_q = Q best_lag, or with polarity Q pick_polarity of the
    correlation that `lags` returns."""
    n = len(as_)
    if n == 0:
        return np.zeros(0, np.int64), np.ones(0, np.int32)
    if frac:
        lag_q, sign = lags_frac(as_, bs, max_lag, Q, W, polarity, batch)
        return np.asarray(lag_q, np.int64).reshape(-1), np.asarray(sign, np.int32).reshape(-1)
    if polarity:
        _, cs = lags(as_, bs, max_lag, batch, return_xcorr=True)
        picked = [pick_polarity(c) for c in cs]
        return np.array([l for l, _ in picked], np.int64).reshape(-1) * int(Q), np.array([g for _, g in picked], np.int32).reshape(-1)
    return np.asarray(lags(as_, bs, max_lag, batch), np.int64).reshape(-1) * int(Q), np.ones(n, np.int32)


def lag_text(lag_q: int, Q: int) -> str:
    """lag_q / Q in samples, printed in full (an exact binary fraction when Q is a power of two); whole lags print as integers."""
    return str(int(lag_q) // int(Q)) if int(lag_q) % int(Q) == 0 else repr(int(lag_q) / int(Q))


def align_pairs(xs, ys, max_lag, frac: bool = False, polarity: bool = False, Q: int = FRAC_Q, W: int = FRAC_W, batch: int = 8, names=None,
                lags=lags_batch, lags_frac=lags_batch_frac, shift=shift_batch, err=None):
    """The --align of estimate_cli and loss_cli: every coded y against its clean x, both cut to the common support -> (xs, ys, lag_q
    int64 [n], sign int32 [n]).  The warnings for a lag at the edge of the search and for an empty support go to `err` (default
    sys.stderr); the caller prints pair_summary of all its calls once."""
    err = err or sys.stderr
    M = _max_lag(max_lag)
    lag_q, sign = find_lags(xs, ys, M, frac, polarity, Q, W, batch, lags, lags_frac)
    windows = []
    for i, (x, y) in enumerate(zip(xs, ys)):
        who = names[i] if names else "pair %d" % i
        if abs(int(lag_q[i])) == M * int(Q):
            print(f"warning: {who}: lag = {lag_text(lag_q[i], Q)} is at the edge of the search (+-{M} samples): the true delay may lie outside it "
                  f"(a larger --align)", file=err)
        n0, n1 = common_support_frac(x.shape[-1], (y.shape[-1],), (lag_q[i],), Q, W)
        if n1 <= n0:
            print(f"warning: {who}: the common support of the aligned signals is empty (lag {lag_text(lag_q[i], Q)}; clean {x.shape[-1]}, coded "
                  f"{y.shape[-1]} samples)", file=err)
        windows.append((n0, max(n1, n0)))
    cut_y = cut_frac(ys, lag_q, sign, windows, Q, W, shift, batch)
    cut_x = [x[..., n0:n1] for x, (n0, n1) in zip(xs, windows)]
    return cut_x, cut_y, lag_q, sign


def add_pair_arguments(p) -> None:
    """The alignment switches of estimate_cli and loss_cli on an argparse parser (eval_cli's names)."""
    p.add_argument("--align", type=float, default=None, metavar="MS",
                   help="after loading, find the delay of every coded file against its clean file within +-MS milliseconds (peak of the "
                        "cross-correlation, on the GPU) and cut both to their common support")
    p.add_argument("--align-frac", action="store_true", help="with --align MS: delays on a grid of 1 / Q samples, the coded file read through a "
                   "windowed-sinc interpolator")
    p.add_argument("--align-polarity", action="store_true", help="with --align MS: pick the peak of |c| and undo an inverted polarity")
    p.add_argument("--align-q", type=int, default=FRAC_Q, metavar="Q", help="--align-frac: grid steps per sample (2 to 1024)")
    p.add_argument("--align-taps", type=int, default=FRAC_W, metavar="W", help="--align-frac: the interpolator has 2 W taps (W from 1 to 256)")


class PairAligner:
    """What --align MS [--align-frac] [--align-polarity] does to the pairs of a run: call it on batches of loaded (xs, ys), then print
    summary() once.  ValueError for switches that do not fit together or a search outside [1, 2^20] samples."""

    def __init__(self, args, sr: int, batch: int, device="cuda", lags=lags_batch, lags_frac=lags_batch_frac, shift=shift_batch):
        if args.align is None:
            raise ValueError("--align-frac and --align-polarity need --align MS")
        M = int(round(float(args.align) * sr / 1000.0)) if np.isfinite(args.align) else 0
        if M < 1 or M > MAX_LAG_CAP:
            raise ValueError(f"--align {args.align:g} ms is {M} samples at {sr} Hz: the search takes 1 to {MAX_LAG_CAP} samples")
        self.M, self.frac, self.polarity, self.batch, self.device = M, bool(args.align_frac), bool(args.align_polarity), max(int(batch), 1), device
        self.Q, self.W = _grid(args.align_q, args.align_taps)
        self.fns = (lags, lags_frac, shift)
        self.lag_q, self.sign = [], []

    def __call__(self, xs, ys, names=None):
        with torch.cuda.device(self.device) if self.device is not None else contextlib.nullcontext():
            xs, ys, lag_q, sign = align_pairs(xs, ys, self.M, self.frac, self.polarity, self.Q, self.W, self.batch, names, *self.fns)
        self.lag_q.extend(int(l) for l in lag_q)
        self.sign.extend(int(g) for g in sign)
        return xs, ys

    def summary(self) -> str:
        return pair_summary(self.lag_q, self.sign, self.Q)


def pair_summary(lag_q, sign, Q: int) -> str:
    """The one alignment summary line of a run of estimate_cli / loss_cli."""
    lag_q, sign = np.asarray(lag_q, np.int64).reshape(-1), np.asarray(sign).reshape(-1)
    lo, hi = (lag_text(lag_q.min(), Q), lag_text(lag_q.max(), Q)) if len(lag_q) else ("0", "0")
    return (f"align: lag min = {lo}  max = {hi} samples (coded against clean, positive = late), non-zero in {int(np.count_nonzero(lag_q))} of "
            f"{len(lag_q)} pairs, {int(np.count_nonzero(sign < 0))} inverted")
