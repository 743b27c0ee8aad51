"""Alignment in time of the three signals of a triple before they are scored: a bounded-lag cross-correlation, the lag of its peak, and the
cut to the common support.  Host yardsticks in NumPy float64 and the GPU path over ragged batches (csrc/xcorr.hip, include/flowdec_hip.h
"Evaluation metrics"), which flowdec_amd/eval_cli.py runs for --align.

* xcorr           c[l + M] = sum_n a[n] b[n + l] for l in [-M, M], n over max(0, -l) <= n < min(La, Lb - l); an empty range is exactly 0.0.
                  The signals are float32, products and sums float64.  A peak at l > 0 means b is a delayed by l samples.
* pick_lag        the l with the largest c, NaN counting as -inf; among equal maxima the smallest |l|, and of -l and +l it is +l; all NaN
                  or all equal (two silent signals) gives 0
* common_support  n0 = max(0, -lag_h, -lag_y), n1 = min(Lx, Lh - lag_h, Ly - lag_y): the samples n of x for which x_hat[n + lag_h] and
                  y[n + lag_y] exist
* align_triple    the three views on that support: equal lengths, no copy, no zero fill

What is left out: fractional delays, clock drift, polarity and gain matching.

Imports `_lib` and `batching` only (no command line).
"""
import numpy as np
import torch

from . import _lib as L
from .batching import length_sorted_batches, padded_rows

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


def lags_batch(as_, bs, max_lag, batch: int = 8, device="cuda", return_xcorr: bool = False):
    """best_lag of every (a, b) on the GPU: lists of 1-D signals of any lengths (the two of a pair may differ) -> int64 [n] (with
    return_xcorr also the float64 [n, 2 M + 1] correlations).  Sorted by the longer signal's length and cut into batches of `batch` pairs;
    each list is staged as zero-padded rows of its own length (batching.padded_rows); a pair's numbers do not depend on its batch."""
    lib = L.load()
    M = _max_lag(max_lag)
    as_, bs = _pairs(as_, bs)
    W = 2 * M + 1
    lags = np.zeros(len(as_), np.int64)
    cs = np.zeros((len(as_), W), np.float64) if return_xcorr else None
    la, lb = [int(c.numel()) for c in as_], [int(c.numel()) for c in bs]
    with torch.cuda.device(device):
        for idx in length_sorted_batches([max(p, q) for p, q in zip(la, lb)], batch):
            B, La, Lb = len(idx), max(max(la[i] for i in idx), 1), max(max(lb[i] for i in idx), 1)
            rows_a, lens_a = padded_rows([as_[i] for i in idx], La, device)
            rows_b, lens_b = padded_rows([bs[i] for i in idx], Lb, device)
            nws = lib.fd_xcorr_workspace_bytes(B, La, Lb, M)
            ws = torch.empty(nws, dtype=torch.uint8, device=device)
            out = torch.empty(B, dtype=torch.int32, device=device)
            c = torch.empty(B, W, dtype=torch.float64, device=device) if return_xcorr else None
            L.check(lib.fd_xcorr_lags(L.ptr(rows_a), L.ptr(rows_b), L.ptr(lens_a), L.ptr(lens_b), B, La, Lb, M, L.ptr(c), L.ptr(out), L.ptr(ws), nws,
                                      L.stream()))
            lags[idx] = out.cpu().numpy()
            if return_xcorr:
                cs[idx] = c.cpu().numpy()
    return (lags, cs) if return_xcorr else lags
