"""NumPy restatement of the resampling contract of include/flowdec_hip.h ("Resampling").

With o = orig / gcd, n = new / gcd, K = 2 width + o and the float32 bank h[n][K] of `audio.sinc_resample_kernel`, output
m = q n + i of an input of L samples is
    acc = 0.0 (float64);  for k = 0 .. K-1 ascending:  j = q o + k - width;  if 0 <= j < L: acc += float64(h[i][k]) * float64(x[j])
    y[m] = float32(acc)
A float32 product is exact in float64, so the float64 add is the loop's only rounding.  The loop over k is explicit, the outputs are
vectorised; a tap outside [0, L) contributes a zero product (acc starts at +0.0: the same bits as skipping it).
"""
import numpy as np


def out_length(L, o, n):
    return -(-int(n) * int(L) // int(o))


def resample(bank, o, n, width, x, x0=0, total=None, m0=0, count=None):
    """The outputs [m0, m0 + count) of a recording of `total` samples (None with x0 = 0: len(x); -1: not known, no upper bound) of which
    `x` (float32, 1-D) holds the samples [x0, x0 + len(x)).  count=None: everything from m0 to ceil(n total / o).  A tap inside the
    recording that `x` does not hold is an error."""
    if total is None:
        assert x0 == 0
        total = len(x)
    if count is None:
        assert total >= 0
        count = out_length(total, o, n) - m0
    bank, x = np.asarray(bank), np.asarray(x)
    K = 2 * width + o
    assert bank.dtype == np.float32 and bank.shape == (n, K) and x.dtype == np.float32 and x.ndim == 1
    m = m0 + np.arange(count, dtype=np.int64)
    q, i = m // n, m % n
    acc = np.zeros(count, dtype=np.float64)
    for k in range(K):
        j = q * o + (k - width)
        inside = (j >= 0) & ((j < total) if total >= 0 else True)
        assert np.all(~inside | ((j >= x0) & (j < x0 + len(x)))), "the span reads a sample x does not hold"
        xv = np.where(inside, x[np.clip(j - x0, 0, max(len(x) - 1, 0))] if len(x) else np.float32(0), np.float32(0)).astype(np.float64)
        acc = acc + bank[i, k].astype(np.float64) * xv
    return acc.astype(np.float32)


def abs_sum(bank, o, n, width, x):
    """sum_k |h x| per output in float64 (the scale of the any-order float32 accumulation bound)."""
    L = len(x)
    count = out_length(L, o, n)
    m = np.arange(count, dtype=np.int64)
    q, i = m // n, m % n
    acc = np.zeros(count, dtype=np.float64)
    xa = np.abs(np.asarray(x, dtype=np.float64))
    for k in range(2 * width + o):
        j = q * o + (k - width)
        inside = (j >= 0) & (j < L)
        acc += np.abs(bank[i, k].astype(np.float64)) * np.where(inside, xa[np.clip(j, 0, max(L - 1, 0))] if L else 0.0, 0.0)
    return acc
