"""What the measurements share on the Python side, without a GPU: the ragged driver of batching.py with a fake `call` on device "cpu",
and the plan cache of _lib.py with a fake maker and a monkeypatched torch.cuda."""
import contextlib

import numpy as np
import pytest
import torch

LENGTHS = [5, 1, 9, 5, 2]


def _clips(lengths, scale=1.0):
    return [torch.arange(1, n + 1, dtype=torch.float32) * (k + 1) * scale for k, n in enumerate(lengths)]


def test_ragged_batches_with_a_fake_call():
    from flowdec_amd.batching import as_clips, length_sorted_batches, ragged_batches
    xs, ys = as_clips(_clips(LENGTHS), [c.numpy() * -1.0 for c in _clips(LENGTHS)])
    want_batches = length_sorted_batches(LENGTHS, 2)
    assert want_batches == [[1, 4], [0, 3], [2]]
    seen = []
    sums, pairs = np.full(5, np.nan), np.full((5, 2, 3), np.nan)          # two outputs of different shapes

    def call(rows, lens, idx, Lrow):
        seen.append(list(idx))
        assert Lrow == max(LENGTHS[i] for i in idx) and lens.dtype == torch.int32 and lens.tolist() == [LENGTHS[i] for i in idx]
        for r, sign in zip(rows, (1.0, -1.0)):
            assert r.dtype == torch.float32 and r.shape == (len(idx), Lrow) and not r.is_cuda
            for k, i in enumerate(idx):
                assert torch.equal(r[k, :LENGTHS[i]], sign * _clips(LENGTHS)[i])
                assert torch.equal(r[k, LENGTHS[i]:], torch.zeros(Lrow - LENGTHS[i]))            # exactly 0.0 behind the clip
        s = rows[0].sum(dim=1).numpy()
        return [s, np.stack([np.full((2, 3), float(i)) for i in idx])]

    ragged_batches((xs, ys), 2, "cpu", call, [sums, pairs], host_call=True)
    assert seen == want_batches
    assert sums.tolist() == [float(c.sum()) for c in _clips(LENGTHS)]                              # every output in its clip's row
    assert all(np.array_equal(pairs[i], np.full((2, 3), float(i))) for i in range(5))
    # the batch order does not matter: one batch of all gives the same rows
    again = np.full(5, np.nan)
    ragged_batches((xs,), 8, "cpu", lambda rows, lens, idx, Lrow: [rows[0].sum(dim=1).numpy()], [again], host_call=True)
    assert np.array_equal(again, sums)
    # a list takes per-clip objects
    boxed = [None] * 5
    ragged_batches((xs,), 2, "cpu", lambda rows, lens, idx, Lrow: [[rows[0][k, :LENGTHS[i]].clone() for k, i in enumerate(idx)]], [boxed], host_call=True)
    assert all(torch.equal(b, c) for b, c in zip(boxed, _clips(LENGTHS)))


def test_ragged_batches_own_rows():
    """Pairs whose two signals differ in length: each list at its own row length, at least 1; sorted by the pair's maximum."""
    from flowdec_amd.batching import ragged_batches
    pair_lengths = [(0, 3), (4, 1), (2, 2)]
    as_ = [torch.full((p,), 1.0 + i) for i, (p, _) in enumerate(pair_lengths)]
    bs = [torch.full((q,), -1.0 - i) for i, (_, q) in enumerate(pair_lengths)]
    seen = []
    out = np.full((3, 2), np.nan)

    def call(rows, lens, idx, Lrow):
        seen.append((list(idx), list(Lrow)))
        assert [r.shape for r in rows] == [(len(idx), Lrow[0]), (len(idx), Lrow[1])]
        assert lens[0].tolist() == [pair_lengths[i][0] for i in idx] and lens[1].tolist() == [pair_lengths[i][1] for i in idx]
        return [torch.stack([rows[0].sum(dim=1), rows[1].sum(dim=1)], dim=1).numpy()]

    ragged_batches((as_, bs), 1, "cpu", call, [out], own_rows=True, host_call=True)
    # maxima 3, 4, 2 -> order 2, 0, 1; the empty signal of pair 0 gets a row of one zero
    assert seen == [([2], [2, 2]), ([0], [1, 3]), ([1], [4, 1])]
    assert out.tolist() == [[0.0, -3.0], [8.0, -2.0], [6.0, -6.0]]
    seen.clear()
    ragged_batches((as_, bs), 2, "cpu", call, [out], own_rows=True, host_call=True)
    assert seen == [([2, 0], [2, 3]), ([1], [4, 1])]
    assert out.tolist() == [[0.0, -3.0], [8.0, -2.0], [6.0, -6.0]]


def test_ragged_batches_refuses_a_cpu_device_for_a_native_call():
    """Without host_call the rows go to a kernel: device "cpu" is refused before anything is staged or called, as the batch functions
    (si_sxr_batch(device="cpu"), lags_batch(device="cpu"), ...) always refused it."""
    from flowdec_amd import align
    from flowdec_amd.batching import ragged_batches
    called = []
    with pytest.raises(ValueError, match="Expected a cuda device, but got: cpu"):
        ragged_batches((_clips(LENGTHS),), 2, "cpu", lambda *a: called.append(a), [np.zeros(5)])
    assert called == []
    with pytest.raises(ValueError, match="Expected a cuda device, but got: cpu"):
        align.lags_batch(_clips([5, 7]), _clips([6, 3]), 2, device="cpu")


def test_as_clips_refusals():
    from flowdec_amd import metrics
    from flowdec_amd.batching import as_clips
    assert metrics.as_clips is as_clips and callable(metrics.length_sorted_batches)
    got = as_clips([np.zeros((1, 3), np.float32)], [torch.ones(3)])
    assert [g[0].shape for g in got] == [(3,), (3,)]
    with pytest.raises(ValueError) as e:
        as_clips([torch.ones(3)], [torch.ones(3), torch.ones(2)])
    assert str(e.value) == "metrics: the lists must have one entry per clip each"
    with pytest.raises(ValueError) as e:
        as_clips([torch.ones(3), torch.ones(4)], [torch.ones(3), torch.ones(5)])
    assert str(e.value) == "metrics: the signals of clip 1 differ in length ([4, 5])"
    with pytest.raises(ValueError) as e:
        as_clips([torch.ones(3), torch.ones(0)], [torch.ones(3), torch.ones(0)])
    assert str(e.value) == "metrics: clip 1 is empty"


@pytest.fixture
def fake_cuda(monkeypatch):
    """torch.cuda with a settable current device and a device context that records itself: state['current'], state['inside']."""
    state = {"current": 0, "inside": None}

    @contextlib.contextmanager
    def device(dev):
        prev, state["inside"] = state["inside"], torch.device(dev)
        try:
            yield
        finally:
            state["inside"] = prev

    monkeypatch.setattr(torch.cuda, "current_device", lambda: state["current"])
    monkeypatch.setattr(torch.cuda, "device", device)
    return state


def test_cuda_device_resolution(fake_cuda):
    from flowdec_amd import _lib as L
    assert L.cuda_device("cuda") == torch.device("cuda", 0)
    fake_cuda["current"] = 1
    assert L.cuda_device("cuda") == torch.device("cuda", 1) and L.cuda_device(torch.device("cuda")) == torch.device("cuda", 1)
    assert L.cuda_device("cuda:0") == torch.device("cuda", 0) and L.cuda_device(torch.device("cuda", 3)).index == 3
    assert L.cuda_device("cpu") == torch.device("cpu")


def test_cached_plan_per_device_and_key(fake_cuda, monkeypatch):
    from flowdec_amd import _lib as L
    monkeypatch.setattr(L, "_PLANS", {})
    made = []

    def maker():
        made.append(fake_cuda["inside"])                       # the device context the maker runs in
        return object()

    key = ("fake", 512, 128)
    p0 = L.cached_plan("cuda", key, maker)
    fake_cuda["current"] = 1
    p1 = L.cached_plan("cuda", key, maker)
    assert p0 is not p1                                         # "cuda" under device 0 and under device 1: two plans
    assert L.cached_plan("cuda:1", key, maker) is p1 and L.cached_plan(torch.device("cuda", 1), key, maker) is p1
    assert L.cached_plan("cuda:0", key, maker) is p0
    assert made == [torch.device("cuda", 0), torch.device("cuda", 1)]          # made once each, inside the resolved device
    assert L.cached_plan("cuda", ("fake", 512, 64), maker) not in (p0, p1) and len(made) == 3


def test_cached_plan_and_a_cpu_device(monkeypatch):
    """A device that is not a GPU: torch.cuda.device refuses it before the maker runs, as every plan function but get_resampler always
    did; with enter=False there is no device context and no call into torch.cuda, and what the maker does with the device stands.
    get_resampler on "cpu" is what it always was: the identity for equal rates, the Resampler's own refusal otherwise."""
    from flowdec_amd import _lib as L
    from flowdec_amd.resample import get_resampler
    monkeypatch.setattr(L, "_PLANS", {})
    made = []
    with pytest.raises(ValueError, match="Expected a cuda device, but got: cpu"):
        L.cached_plan("cpu", ("fake",), lambda: made.append(0) or object())
    assert made == [] and L._PLANS == {}

    def touched(*a, **k):
        raise AssertionError("torch.cuda was touched for a cpu device")

    monkeypatch.setattr(torch.cuda, "current_device", touched)
    monkeypatch.setattr(torch.cuda, "device", touched)
    p = L.cached_plan("cpu", ("fake",), lambda: made.append(1) or object(), enter=False)
    assert L.cached_plan(torch.device("cpu"), ("fake",), lambda: made.append(1) or object(), enter=False) is p and made == [1]
    r = get_resampler(48000, 48000, device="cpu")
    assert r.identity and r.device == torch.device("cpu") and r.out_length(777) == 777 and get_resampler(16000, 16000, device="cpu") is r
    x = torch.arange(5.0)
    assert r(x) is x
    with pytest.raises(RuntimeError) as e:
        get_resampler(44100, 48000, device="cpu")
    assert str(e.value) == "flowdec_amd: Resampler runs on the GPU (HIP is the only compute path)"
    assert all(k[1][0] != "resample" or v.identity for k, v in L._PLANS.items())          # the refused plan was not cached


def test_stft_plan_follows_the_current_device(fake_cuda, monkeypatch):
    """ops.stft_plan("cuda") after the current device changed: the new device's plan, not the first one's."""
    from flowdec_amd import _lib as L, ops
    monkeypatch.setattr(L, "_PLANS", {})
    made = []

    def make(n_fft, hop):
        made.append((fake_cuda["inside"], n_fft, hop))
        return L.Handle("fd_stft_plan_destroy")                 # (an empty handle: nothing to free)

    monkeypatch.setattr(ops, "_make_stft_plan", make)
    h0 = ops.stft_plan(512, 128, "cuda")
    fake_cuda["current"] = 1
    h1 = ops.stft_plan(512, 128, "cuda")
    assert h0 is not h1 and ops.stft_plan(512, 128, "cuda:1") is h1 and ops.stft_plan(512, 128, "cuda:0") is h0
    assert made == [(torch.device("cuda", 0), 512, 128), (torch.device("cuda", 1), 512, 128)]


def test_handle_frees_once_and_swallows(monkeypatch):
    import ctypes as C
    from flowdec_amd import _lib as L
    freed = []

    class Lib:
        @staticmethod
        def fd_fake_destroy(h):
            freed.append(h.value)

        @staticmethod
        def fd_fake_broken(h):
            raise RuntimeError("interpreter exit")

    monkeypatch.setattr(L, "load", lambda: Lib)
    L.Handle("fd_fake_destroy").__del__()                       # an empty handle: nothing to free
    h = L.Handle("fd_fake_destroy")
    h.handle = C.c_void_p(77)
    del h
    assert freed == [77]
    b = L.Handle("fd_fake_broken")
    b.handle = C.c_void_p(5)
    b.__del__()                                                 # swallowed
