"""What the measurements share, on the GPU: the plan cache gives one plan for "cuda" and for the current device by index, and
fd_xcorr_lags is fd_xcorr_lags_frac without polarity up to the last kernel (one slice kernel, one finalise kernel: csrc/xcorr.hip)."""
import numpy as np
import pytest

from test_hip_align import gpu_xcorr
from test_hip_align_frac import Q, W, gpu_frac, noise_pair, same_bits

pytestmark = pytest.mark.gpu

PAIRS = ((1, 5), (300, 257), (5000, 4000))        # samples of a, of b
WHOLE = {1: (0, 1, 2), 200: (1, 2)}               # max_lag -> the pairs whose refined peak is the whole-sample delay of 1


def test_one_plan_for_cuda_and_for_the_current_device():
    import torch
    from flowdec_amd import metrics, ops, segsnr, specdist
    assert torch.cuda.current_device() == 0
    h = ops.stft_plan(512, 128, "cuda")
    assert h is ops.stft_plan(512, 128, "cuda:0") and h.value
    assert segsnr.segsnr_plan(16000, "cuda") is segsnr.segsnr_plan(16000, "cuda:0")
    assert specdist.specdist_plan(48000, "cuda") is specdist.specdist_plan(48000, "cuda:0")
    assert metrics.estoi_plans(16000, "cuda") is metrics.estoi_plans(16000, "cuda:0")
    assert metrics.estoi_plans(16000).estoi.value and metrics.estoi_plans(16000).resample.value


@pytest.fixture(scope="module")
def pairs():
    """noise_pair's white noise and its copy one sample later, cut to the two lengths of PAIRS."""
    out = []
    for i, (La, Lb) in enumerate(PAIRS):
        a, b = noise_pair(max(La, Lb), 1, 500 + i)
        out.append((a[:La].copy(), b[:Lb].copy()))
    return out


@pytest.mark.parametrize("M", [1, 200])
def test_whole_sample_lags_are_the_fractional_ones_without_polarity(pairs, M):
    """The c arrays of the two entry points are the same bits, and so is the whole-sample pick: lag_q = Q lags + q with |q| < Q by
    refine_lag's rule (exact, from the device's own c), and for the pairs of WHOLE[M], whose refined peak the host yardstick puts on a
    whole sample, lag_q // Q is lags itself and lag_q has no fraction.  The one pair left out: a single sample against five at M = 200,
    where c is that sample times the other signal, white noise, and its interpolation peaks between two samples."""
    from flowdec_amd import align
    c_int, lags = gpu_xcorr(pairs, M)
    c_frac, lag_q, sign = gpu_frac(pairs, M, False)
    assert same_bits(c_int, c_frac)
    for i, (a, b) in enumerate(pairs):
        assert (int(lag_q[i]), int(sign[i])) == align.refine_lag(c_frac[i], Q, W, False), (PAIRS[i], M)
        assert abs(int(lag_q[i]) - int(lags[i]) * Q) < Q and sign[i] == 1, (PAIRS[i], M, lag_q[i], lags[i])
        host_whole = align.refine_lag(align.xcorr(a, b, M), Q, W, False)[0] % Q == 0
        assert host_whole == (i in WHOLE[M]), (PAIRS[i], M)                      # (the premise, on the host)
        if i in WHOLE[M]:
            assert lag_q[i] % Q == 0 and lag_q[i] // Q == lags[i] == 1, (PAIRS[i], M, lag_q[i], lags[i])
    assert np.array_equal(lags, [align.pick_lag(c) for c in c_int])
