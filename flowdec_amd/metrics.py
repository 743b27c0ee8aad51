"""Parity metrics between two waveforms: the reference's own evaluation formulas, used here
to express build-vs-reference differences in the units the paper reports.  Host-side NumPy / torch-CPU, not on the hot path.

* si_sxr      -- SI-SDR / SI-SIR / SI-SAR (flowdec/eval/metrics.py:256-270, components :554-563); pinned by
                 tests/golden/g14_metrics.npz (reference code run on seeded signals).
* logspec_mse -- mean squared error of 10*log10 power spectrograms, 32 ms symmetric-Hann window / 8 ms hop
                 (eval/metrics.py:333-372).  The reference computes the spectrogram with torchaudio, which is not in
                 this image: restated with torch.stft, parity unpinned.

The two of them also run on the GPU over ragged batches (csrc/metrics.hip, include/flowdec_hip.h "Evaluation metrics"): si_sxr_batch and
logspec_mse_batch below, which score a triples list in flowdec_amd/eval_cli.py.  The host functions stay the yardstick of those.
"""
import numpy as np
import torch


def _flat(a) -> np.ndarray:
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    return np.asarray(a, dtype=np.float64).reshape(-1) if np.asarray(a).dtype == np.float64 else np.asarray(a).reshape(-1)


def si_sxr_components(s_hat, s, n):
    s_target = (np.dot(s_hat, s) / np.linalg.norm(s) ** 2) * s
    e_noise = (np.dot(s_hat, n) / np.linalg.norm(n) ** 2) * n
    return s_target, e_noise, s_hat - s_target - e_noise


def si_sxr(x_hat, x, y):
    """-> (si_sdr, si_sir, si_sar) in dB; x = reference signal, y = degraded input (noise n = y - x, or y + x when that has
    less power: the reference's global-phase-flip guard)."""
    x_hat, x, y = _flat(x_hat), _flat(x), _flat(y)
    n = y - x
    if np.linalg.norm(y + x) < np.linalg.norm(y - x):
        n = y + x
    s_target, e_noise, e_art = si_sxr_components(x_hat, x, n)
    p = np.linalg.norm(s_target) ** 2
    return (10 * np.log10(p / np.linalg.norm(e_noise + e_art) ** 2), 10 * np.log10(p / np.linalg.norm(e_noise) ** 2),
            10 * np.log10(p / np.linalg.norm(e_art) ** 2))


def si_sdr(x_hat, x) -> float:
    """Plain scale-invariant SDR of x_hat against x (no noise decomposition), for build-vs-reference comparisons."""
    x_hat, x = _flat(x_hat).astype(np.float64), _flat(x).astype(np.float64)
    s_target = (np.dot(x_hat, x) / np.dot(x, x)) * x
    return float(10 * np.log10(np.dot(s_target, s_target) / max(np.dot(x_hat - s_target, x_hat - s_target), 1e-300)))


def logspec_mse(x_hat, x, sr: int = 48000, win_dur: float = 32e-3, hop_dur: float = 8e-3, eps: float = 1e-8) -> float:
    n_fft, hop = int(win_dur * sr), int(hop_dur * sr)
    win = torch.signal.windows.hann(n_fft)

    def logspec(a):
        a = torch.as_tensor(np.asarray(_flat(a), dtype=np.float32))
        S = torch.stft(a, n_fft, hop_length=hop, win_length=n_fft, window=win, center=True, pad_mode="reflect", return_complex=True)
        return 10 * torch.log10(torch.clamp(S.abs() ** 2, min=eps))
    return float(torch.mean(torch.square(logspec(x) - logspec(x_hat))))


# ---- the same two metrics on the GPU, over ragged batches (csrc/metrics.hip) -------------------------------------------------------------
SISXR_SUMS = ("x.x", "x_hat.x", "x_hat.n", "n.n", "|s_target|^2", "|e_noise|^2", "|e_art|^2", "|e_noise+e_art|^2")   # fd_metrics_sisxr


def sisxr_from_sums(sums) -> np.ndarray:
    """[n, 8] float64 sums of fd_metrics_sisxr (layout SISXR_SUMS) -> [n, 3] float64 (si_sdr, si_sir, si_sar) in dB, formed on the host."""
    s = np.asarray(sums, dtype=np.float64).reshape(-1, 8)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.stack([10 * np.log10(s[:, 4] / s[:, 7]), 10 * np.log10(s[:, 4] / s[:, 5]), 10 * np.log10(s[:, 4] / s[:, 6])], axis=1)


def length_sorted_batches(lengths, batch: int):
    """Indices sorted by length (ties by index) and cut into batches of at most `batch`: the clips of one call have similar lengths, so
    little of a row is padding.  The results do not depend on this (a clip's bits are the same in any batch)."""
    order = sorted(range(len(lengths)), key=lambda i: (lengths[i], i))
    batch = max(int(batch), 1)
    return [order[i:i + batch] for i in range(0, len(order), batch)]


def _rows(clips, idx, device):
    """-> (rows [B, Lmax] float32 on the device, zero behind each clip; lengths int32 [B] on the device)."""
    Lmax = max(int(clips[i].numel()) for i in idx)
    rows = torch.zeros(len(idx), Lmax, dtype=torch.float32)
    for r, i in enumerate(idx):
        rows[r, :clips[i].numel()] = clips[i].detach().reshape(-1).float().cpu()
    return rows.to(device)


def _as_clips(*lists):
    out = [[torch.as_tensor(c).reshape(-1) for c in l] for l in lists]
    n = len(out[0])
    for l in out[1:]:
        if len(l) != n:
            raise ValueError("metrics: the lists must have one entry per clip each")
    for i in range(n):
        if len({int(l[i].numel()) for l in out}) != 1:
            raise ValueError(f"metrics: the signals of clip {i} differ in length ({[int(l[i].numel()) for l in out]})")
        if out[0][i].numel() < 1:
            raise ValueError(f"metrics: clip {i} is empty")
    return out


def si_sxr_sums_batch(x_hats, xs, ys, batch: int = 8, device="cuda") -> np.ndarray:
    """The float64 sums of fd_metrics_sisxr per clip, [n, 8] (layout SISXR_SUMS)."""
    from . import _lib as L
    lib = L.load()
    x_hats, xs, ys = _as_clips(x_hats, xs, ys)
    out = np.zeros((len(xs), 8), np.float64)
    lengths = [int(c.numel()) for c in xs]
    with torch.cuda.device(device):
        for idx in length_sorted_batches(lengths, batch):
            h, x, y = (_rows(l, idx, device) for l in (x_hats, xs, ys))
            lens = torch.tensor([lengths[i] for i in idx], dtype=torch.int32, device=device)
            B, Lmax = x.shape
            nws = lib.fd_metrics_workspace_bytes(B, Lmax, 0, 0)
            ws = torch.empty(nws, dtype=torch.uint8, device=device)
            sums = torch.empty(B, 8, dtype=torch.float64, device=device)
            L.check(lib.fd_metrics_sisxr(L.ptr(h), L.ptr(x), L.ptr(y), L.ptr(lens), B, Lmax, L.ptr(sums), L.ptr(ws), nws, L.stream()))
            out[idx] = sums.cpu().numpy()
    return out


def si_sxr_batch(x_hats, xs, ys, batch: int = 8, device="cuda") -> np.ndarray:
    """si_sxr of every (x_hat, x, y) on the GPU: lists of 1-D signals of any lengths -> [n, 3] float64 (si_sdr, si_sir, si_sar) in dB.
    Sorted by length, cut into batches of `batch` clips, summed in float64 on the device (two passes), dB formed here."""
    return sisxr_from_sums(si_sxr_sums_batch(x_hats, xs, ys, batch, device))


def logspec_mse_batch(x_hats, xs, sr: int = 48000, win_dur: float = 32e-3, hop_dur: float = 8e-3, eps: float = 1e-8, batch: int = 8,
                      device="cuda") -> np.ndarray:
    """logspec_mse of every (x_hat, x) on the GPU -> [n] float64.  One cached transform plan per (n_fft, hop) (ops.stft_plan).  A clip of
    n_fft / 2 samples or fewer cannot be reflect-padded (torch.stft raises): ValueError naming the clip."""
    from . import _lib as L, ops
    lib = L.load()
    n_fft, hop = int(win_dur * sr), int(hop_dur * sr)
    x_hats, xs = _as_clips(x_hats, xs)
    lengths = [int(c.numel()) for c in xs]
    for i, l in enumerate(lengths):
        if l <= n_fft // 2:
            raise ValueError(f"logspec_mse: clip {i} has {l} samples, reflect padding of n_fft {n_fft} needs more than {n_fft // 2}")
    out = np.zeros(len(xs), np.float64)
    plan = ops.stft_plan(n_fft, hop, device)
    with torch.cuda.device(device):
        for idx in length_sorted_batches(lengths, batch):
            h, x = (_rows(l, idx, device) for l in (x_hats, xs))
            lens = torch.tensor([lengths[i] for i in idx], dtype=torch.int32, device=device)
            B, Lmax = x.shape
            nws = lib.fd_metrics_workspace_bytes(B, Lmax, n_fft, hop)
            ws = torch.empty(nws, dtype=torch.uint8, device=device)
            mse = torch.empty(B, dtype=torch.float64, device=device)
            L.check(lib.fd_metrics_logspec_mse(plan, L.ptr(h), L.ptr(x), L.ptr(lens), B, Lmax, float(eps), L.ptr(mse), L.ptr(ws), nws, L.stream()))
            out[idx] = mse.cpu().numpy()
    return out
