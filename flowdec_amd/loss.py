"""Validation loss of a checkpoint on (clean, coded) pairs: the quantity the reference's `validation_step` logs as `valid_loss`
(flowdec/model.py:221-223), i.e. `_loss` of FlowModel (:421-468), ScoreModel (:590-611) and RegressionModel (:552-559) without gradients.

One native call per batch (fd_valid_loss, include/flowdec_hip.h "Validation loss"): the pair front end `_preprocess(y, x=x)`, the random
draws, ONE network evaluation at a per-clip random time and per-clip sums of |err|^2 in float64.  What is left on the host is the
reduction of a handful of float64 numbers, restated here from the reference:

* flow        per-clip mean over the F * T_pad bins; clips whose value is NaN are dropped with a warning, ValueError if all are; then the
              mean over the clips (:444-467)
* score       0.5 * mean over the clips of the per-clip SUM (:608-610)
* regression  mean over every bin of every clip (:558)

The draws: `seed=` uses the library's counter-based noise ("Seeded noise": draw 0 for Ys / Zs, draw 1 for Xs) and draws the time t from
the same seed (fd_loss_times); `noise=` / `t=` inject them; with neither, torch's global generator is used like the reference does.
`FlowModel.valid_loss`, `ScoreModel.valid_loss`, `RegressionModel.valid_loss` and the `valid_loss_batch` forms in flowdec_amd/model.py
are thin wrappers of `valid_loss` / `valid_loss_batch` below; flowdec_amd/loss_cli.py is the command line."""
import ctypes as C
import logging
from typing import Optional, Sequence

import numpy as np
import torch

from . import _lib as L
from . import noise as fd_noise
from .batching import _ragged_bucket, _to_3d, padded_rows, plan_clip_batches

log = logging.getLogger(__name__)


# ---- the three reductions (host, float64) ------------------------------------------------------------------------------------------------
def per_clip_values(kind: str, sums, n_bins) -> np.ndarray:
    """sums [B] (sum |err|^2 of each clip over its n_bins = F * T_pad bins) -> what the reference holds per clip BEFORE its reduction:
    flow / regression the mean over the bins, score the sum.  n_bins: an int or one per clip.  float64."""
    sums = np.asarray(sums, np.float64)
    if kind == "score":
        return sums.copy()
    if kind in ("flow", "regression"):
        return sums / np.asarray(n_bins, np.float64)
    raise ValueError(f"unknown loss kind {kind!r} (flow, score or regression)")


def reduce_values(kind: str, values, names: Optional[Sequence[str]] = None) -> float:
    """The reference's reduction of the per-clip values (per_clip_values) to one loss.  flow: NaN clips are dropped with a warning,
    ValueError if every clip is NaN (model.py:446-467); score: 0.5 * mean; regression: the mean (every clip of a batch has the same number
    of bins there, so the mean of the per-clip means is the mean over everything)."""
    v = np.asarray(values, np.float64).reshape(-1)
    if v.size == 0:
        raise ValueError("valid_loss: no clips")
    if kind == "flow":
        isnan = np.isnan(v)
        if isnan.any():
            bad = [str(names[i]) if names is not None else str(i) for i in np.nonzero(isnan)[0]]
            log.warning("valid_loss: NaN loss for clip(s) %s -- ignoring them", ", ".join(bad))
            if isnan.all():
                raise ValueError("valid_loss: every clip of the batch led to a NaN loss value")
            v = v[~isnan]
        return float(v.mean())
    if kind == "score":
        return float(0.5 * v.mean())
    if kind == "regression":
        return float(v.mean())
    raise ValueError(f"unknown loss kind {kind!r} (flow, score or regression)")


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------
def _config(model, kind: str, comp_eps=None) -> L.FdLossConfig:
    """fd_loss_config of `model`; raises for everything of the reference's `_loss` that this path does not compute."""
    if comp_eps is not None:
        raise NotImplementedError("valid_loss: comp_eps (a training-time regulariser, feature_extractors.py:124-125) is not supported")
    cfg = L.FdLossConfig(kind=L.LOSS_KINDS[kind])
    if kind == "flow":
        fm = getattr(model, "flow_matcher", None)
        if fm is not None and float(getattr(fm, "sigma", 0.0)) != 0.0:
            raise NotImplementedError(f"valid_loss: flow_matcher.sigma = {float(fm.sigma)}: only the ConditionalFlowMatcher with sigma = 0 "
                                      f"(xt = t x1 + (1 - t) x0, ut = x1 - x0) is computed")
        if getattr(model, "error_weighting", None) is not None:
            raise NotImplementedError("valid_loss: error_weighting is not supported (an unused experiment of the reference, model.py:438-441)")
        sx = model.sigma_x
        if callable(sx) and not isinstance(sx, torch.Tensor):
            raise NotImplementedError("valid_loss: a callable sigma_x is not supported (a scalar only)")
        if isinstance(sx, torch.Tensor) and sx.numel() != 1:
            raise NotImplementedError(f"valid_loss: sigma_x must be a scalar (got shape {tuple(sx.shape)})")
        cfg.sigma_x = float(sx)
        if cfg.sigma_x < 0:
            raise ValueError("valid_loss: sigma_x must not be negative")
    elif kind == "score":
        sde = model.sde
        cfg.theta, cfg.sigma_min, cfg.sigma_max, cfg.t_eps = float(sde.theta), float(sde.sigma_min), float(sde.sigma_max), float(model.t_eps)
    return cfg


def time_range(model, kind: str):
    """[lo, hi) of the random time: torch.rand(B) for flow (model.py:428), torch.rand(B) * (T - t_eps) + t_eps for score (:594)."""
    return (float(model.t_eps), 1.0) if kind == "score" else (0.0, 1.0)


def pair_seeds(seeds, n: int):
    """`seeds=` of valid_loss_batch -> one 64-bit seed per pair (a list of ints) or None: an int S seeds pair i of the LIST with
    flowdec_amd.noise.clip_seed(S, i), whatever bucket or native call the pair lands in; a sequence or an int64 / uint64 tensor gives the
    seeds directly."""
    if seeds is None:
        return None
    if isinstance(seeds, torch.Tensor):
        seeds = [int(s) for s in seeds.view(torch.int64).cpu().reshape(-1)]
    elif not isinstance(seeds, (list, tuple)):
        seeds = [fd_noise.clip_seed(int(seeds), i) for i in range(n)]
    if len(seeds) != n:
        raise ValueError(f"valid_loss_batch: one seed per pair: got {len(seeds)} seeds for {n} pairs")
    return [int(s) for s in seeds]


def loss_times(seeds: torch.Tensor, lo: float, hi: float) -> torch.Tensor:
    """fd_loss_times: the per-clip times of the clips seeded `seeds` (int64 [B] on the GPU) -> float32 [B]."""
    L.require_cuda(seeds)
    lib = L.load()
    t = torch.empty(seeds.numel(), dtype=torch.float32, device=seeds.device)
    with torch.cuda.device(seeds.device):
        L.check(lib.fd_loss_times(L.ptr(seeds), seeds.numel(), float(lo), float(hi), L.ptr(t), L.stream()))
    return t


# ---- one native call -----------------------------------------------------------------------------------------------------------------------
def _native(model, kind, cfg, x_rows, y_rows, lens, seeds, noise, t):
    """fd_valid_loss on rows [B, Lrow] that live on the model's device.  lens: int32 [B] on the device (ragged, one T_pad bucket) or None.
    seeds: int64 [B] device | None; noise: complex64 [n_draws, B, 1, F, Tp] device | None; t: float32 [B] device | None.
    -> dict(sums float64 [B], bad int64 [B], normfac float32 [B], t float32 [B] | None (tensors on the device), n_bins)."""
    lib = L.load()
    dev = model.device
    B, Lrow = y_rows.shape
    stft = model.feature_extractor._cfg()
    F = stft["n_fft"] // 2 + 1
    with model._native_call(), torch.cuda.device(dev):
        h = model._sync_native()
        Tp = int(lib.fd_padded_frames(lib.fd_num_frames(Lrow, stft["hop"])))
        need = int(lib.fd_valid_loss_workspace_bytes(h, B, Lrow))
        if need == 0:
            raise RuntimeError(f"valid_loss: no workspace for {B} clips of {Lrow} samples (at most 256 clips per call, each longer than "
                               f"{stft['n_fft'] // 2} samples)")
        ws = model.backbone.workspace(("loss", B, Lrow), need, dev)
        sums = torch.empty(B, dtype=torch.float64, device=dev)
        bad = torch.empty(B, dtype=torch.int64, device=dev)
        normfac = torch.empty(B, dtype=torch.float32, device=dev)
        if kind != "regression" and t is None and seeds is not None:
            t = loss_times(seeds, *time_range(model, kind))
        L.check(lib.fd_valid_loss(h, C.byref(cfg), L.ptr(x_rows), L.ptr(y_rows), L.ptr(lens), None if noise is None else L.ptr(torch.view_as_real(noise)),
                                  L.ptr(seeds), L.ptr(t), L.ptr(sums), L.ptr(bad), L.ptr(normfac), B, Lrow, L.ptr(ws), ws.numel(), L.stream()))
    return dict(sums=sums, bad=bad, normfac=normfac, t=t, n_bins=F * Tp)


def _draws(model, kind, cfg, B, F, Tp, seed, noise, t, dev):
    """The three sources of the draws -> (seeds, noise, t) as fd_valid_loss takes them (device tensors or None)."""
    if kind == "regression":
        if seed is not None or noise is not None or t is not None:
            raise ValueError("valid_loss: the regression loss has no random draws (seed=, noise= and t= do not apply)")
        return None, None, None
    fd_noise.exclusive(seed=seed, noise=noise)
    n_draws = int(L.load().fd_loss_num_draws(C.byref(cfg)))
    lo, hi = time_range(model, kind)
    seeds_dev = None
    if seed is not None:
        seeds_dev = fd_noise.seeds_to_tensor(seed, B, dev)
    elif noise is not None:
        noise = noise.to(dev, torch.complex64)
        if noise.numel() != n_draws * B * F * Tp:
            raise ValueError(f"valid_loss: noise must hold {n_draws} draw(s) of shape [{B}, 1, {F}, {Tp}] (got {tuple(noise.shape)})")
        noise = noise.reshape(n_draws, B, 1, F, Tp).contiguous()
    else:      # the reference's behaviour: the global generator
        noise = torch.randn(n_draws, B, 1, F, Tp, dtype=torch.complex64, device=dev)
    if t is not None:
        t = torch.as_tensor(t, dtype=torch.float32).reshape(-1).to(dev).contiguous()
        if t.numel() != B:
            raise ValueError(f"valid_loss: one time per clip: got {t.numel()} for {B} clips")
    elif seeds_dev is None:
        t = (torch.rand(B, device=dev) * (hi - lo) + lo).contiguous()
    return seeds_dev, noise, t


def _require_gpu(model):
    dev = model.device
    if dev.type != "cuda":
        raise RuntimeError("flowdec_amd: move the model to the GPU first (`model.cuda()`); there is no CPU path")
    return dev


def _finish(model, kind, res, reduce, return_t):
    sums = res["sums"].cpu().numpy()
    values = per_clip_values(kind, sums, res["n_bins"])
    t = None if res["t"] is None else res["t"].cpu()
    model.last_loss_info = dict(sums=sums, per_clip=values, bad=res["bad"].cpu().numpy(), normfac=res["normfac"].cpu(), t=t)
    if reduce == "none":
        out = values
    elif reduce == "mean":
        out = reduce_values(kind, values)
    else:
        raise ValueError(f"valid_loss: reduce must be 'mean' or 'none' (got {reduce!r})")
    return (out, t) if return_t else out


@torch.no_grad()
def valid_loss(model, kind: str, x, y, *, seed=None, noise=None, t=None, reduce: str = "mean", return_t: bool = False, comp_eps=None):
    """`model._loss((x, y, names), ...)` of the reference for clean x and coded y of ONE length: [L], [1, L] or [B, 1, L] (B <= 256).
    -> the loss (a float), or with reduce='none' the per-clip values (float64 [B]: per_clip_values); return_t=True adds the times used
    (float32 [B] on the host; None for regression).  `model.last_loss_info` keeps sums, per_clip, bad (non-finite err elements per clip),
    normfac and t of the call."""
    if reduce not in ("mean", "none"):
        raise ValueError(f"valid_loss: reduce must be 'mean' or 'none' (got {reduce!r})")
    cfg = _config(model, kind, comp_eps)
    x, y = torch.as_tensor(x), torch.as_tensor(y)
    if x.shape != y.shape:
        raise RuntimeError(f"valid_loss: x and y must have the same shape (got {tuple(x.shape)} vs {tuple(y.shape)})")   # model.py:141
    dev = _require_gpu(model)
    y3, _ = _to_3d(y, "valid_loss expects")
    B, Lw = y3.shape[0], y3.shape[-1]
    stft = model.feature_extractor._cfg()
    lib = L.load()
    F, Tp = stft["n_fft"] // 2 + 1, int(lib.fd_padded_frames(lib.fd_num_frames(Lw, stft["hop"])))
    seeds_dev, noise, t = _draws(model, kind, cfg, B, F, Tp, seed, noise, t, dev)
    xr = x.reshape(B, Lw).to(dev, torch.float32).contiguous()
    yr = y3.reshape(B, Lw).to(dev, torch.float32).contiguous()
    return _finish(model, kind, _native(model, kind, cfg, xr, yr, None, seeds_dev, noise, t), reduce, return_t)


@torch.no_grad()
def valid_loss_batch(model, kind: str, xs, ys, *, seeds=None, noise=None, t=None, reduce: str = "mean", return_t: bool = False, max_batch: int = 8):
    """The same for LISTS of clips of any lengths: pair i is (xs[i], ys[i]), [L_i], [1, L_i] or [1, 1, L_i].  The pairs are bucketed by
    their padded frame count (flowdec_amd.model.padded_frames_of) like `enhance_batch`'s callers do, at most `max_batch` per native call;
    every pair's value, time and normfac are BIT-IDENTICAL to its one-pair `valid_loss` call with the same draws, whatever the bucketing.
    seeds: an int (pair i is seeded flowdec_amd.noise.clip_seed(seeds, i)) or one 64-bit seed per pair; noise: one tensor
    [n_draws, 1, F, T_pad_i] per pair; t: one time per pair.  reduce='mean' applies the class's reduction to all per-pair values (pairs of
    different T_pad have different bin counts: the regression mean is then the mean of the per-pair means)."""
    if reduce not in ("mean", "none"):
        raise ValueError(f"valid_loss_batch: reduce must be 'mean' or 'none' (got {reduce!r})")
    cfg = _config(model, kind)
    xs, ys = [torch.as_tensor(c) for c in xs], [torch.as_tensor(c) for c in ys]
    n = len(ys)
    if n < 1 or len(xs) != n:
        raise ValueError(f"valid_loss_batch: {len(xs)} clean and {len(ys)} coded clips (one of each per pair, at least one pair)")
    for i, (a, b) in enumerate(zip(xs, ys)):
        if a.shape != b.shape:
            raise RuntimeError(f"valid_loss_batch: pair {i}: x and y must have the same shape (got {tuple(a.shape)} vs {tuple(b.shape)})")
    dev = _require_gpu(model)
    if kind == "regression":
        if seeds is not None or noise is not None or t is not None:
            raise ValueError("valid_loss_batch: the regression loss has no random draws (seeds=, noise= and t= do not apply)")
    else:
        fd_noise.exclusive(seeds=seeds, noise=noise)
        if noise is not None and len(noise) != n:
            raise ValueError("valid_loss_batch: one noise tensor per pair")
        seeds = pair_seeds(seeds, n)
        if t is not None:
            t = torch.as_tensor(t, dtype=torch.float32).reshape(-1)
            if t.numel() != n:
                raise ValueError(f"valid_loss_batch: one time per pair: got {t.numel()} for {n} pairs")
    stft = model.feature_extractor._cfg()
    F = stft["n_fft"] // 2 + 1
    max_batch = max(1, min(int(max_batch), 256))
    sums, bad = np.zeros(n, np.float64), np.zeros(n, np.int64)
    n_bins = np.zeros(n, np.float64)
    normfac, times = torch.zeros(n, dtype=torch.float32), (None if kind == "regression" else torch.zeros(n, dtype=torch.float32))
    done = []
    for Tp, part in plan_clip_batches([c.shape[-1] for c in ys], stft["hop"], max_batch):
        flat_y, _, _, Lrow = _ragged_bucket([ys[i] for i in part], stft)
        B = len(part)
        (xr, _), (yr, lens) = padded_rows([xs[i].reshape(-1) for i in part], Lrow, dev), padded_rows(flat_y, Lrow, dev)
        if kind == "regression":
            sd = nz = tt = None
        else:
            nz = None if noise is None else torch.stack([torch.as_tensor(noise[i]).to(dev, torch.complex64).reshape(-1, 1, F, Tp) for i in part], dim=1)
            sd, nz, tt = _draws(model, kind, cfg, B, F, Tp, None if seeds is None else [seeds[i] for i in part], nz,
                                None if t is None else t[part], dev)
        done.append((part, _native(model, kind, cfg, xr, yr, lens, sd, nz, tt)))
    for part, res in done:      # read back after the last call is enqueued: no host synchronisation between the native calls
        sums[part], bad[part] = res["sums"].cpu().numpy(), res["bad"].cpu().numpy()
        n_bins[part] = res["n_bins"]
        normfac[part] = res["normfac"].cpu()
        if times is not None:
            times[part] = res["t"].cpu()
    values = per_clip_values(kind, sums, n_bins)
    model.last_loss_info = dict(sums=sums, per_clip=values, bad=bad, normfac=normfac, t=times)
    out = values if reduce == "none" else reduce_values(kind, values)
    return (out, times) if return_t else out
