"""Host-side mirror of the reference's Python API for the inference hot path.

Same names, argument meaning, defaults, return conventions and state_dict key layout as

* ``flowdec.model.FlowModel``            (flowdec/model.py:391-536)  -> :class:`FlowModel`
* ``flowdec.backbones.ncsnpp.NCSNpp``    (flowdec/backbones/ncsnpp.py:49-411) -> :class:`NCSNpp`
* ``flowdec.data.feature_extractors.AmplitudeCompressedComplexSTFT`` (:29-59) -> same name here

but every FLOP runs in libflowdec_hip.so (hand-written HIP for gfx950).  The ``nn.Module`` tree only
holds parameters (so ``load_state_dict(ckpt['_pl_ema_state_dict'])`` works unchanged); there is no
Lightning / Hydra / torchdyn dependency and no PyTorch compute fallback.
"""
import contextlib
import ctypes as C
import math
import os
import threading
from typing import Optional, Sequence, Tuple

import numpy as np
import torch
import torch.nn as nn

from . import _lib as L
from . import longform, ops
from . import loss as fd_loss
from . import noise as fd_noise
from .batching import _ragged_bucket, _to_3d, padded_frames_of, padded_rows  # noqa: F401  (padded_frames_of: the bucket key callers import from here)

_DATA = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data")


# ------------------------------------------------------------------------------------------------
# parameter containers (names/shapes identical to the reference modules)
# ------------------------------------------------------------------------------------------------
class GaussianFourierProjection(nn.Module):
    """layerspp.py:42-51 (parameter container; W is frozen)."""

    def __init__(self, embedding_size=256, scale=1.0):
        super().__init__()
        self.W = nn.Parameter(torch.randn(embedding_size) * scale, requires_grad=False)


class ResnetBlockBigGANpp(nn.Module):
    """layerspp.py:222-284 (parameter container)."""

    def __init__(self, in_ch, out_ch=None, temb_dim=None, up=False, down=False):
        super().__init__()
        out_ch = out_ch if out_ch else in_ch
        self.GroupNorm_0 = nn.GroupNorm(min(in_ch // 4, 32), in_ch, eps=1e-6)
        self.Conv_0 = nn.Conv2d(in_ch, out_ch, 3, padding=1)
        self.Dense_0 = nn.Linear(temb_dim, out_ch)
        self.GroupNorm_1 = nn.GroupNorm(min(out_ch // 4, 32), out_ch, eps=1e-6)
        self.Conv_1 = nn.Conv2d(out_ch, out_ch, 3, padding=1)
        if in_ch != out_ch or up or down:
            self.Conv_2 = nn.Conv2d(in_ch, out_ch, 1)
        self.up, self.down, self.in_ch, self.out_ch = up, down, in_ch, out_ch


class NIN(nn.Module):
    """layers.py:566-575 (parameter container): y = x W + b over the channel axis, W is [in, out]."""

    def __init__(self, in_dim, num_units):
        super().__init__()
        self.W = nn.Parameter(torch.zeros(in_dim, num_units))
        self.b = nn.Parameter(torch.zeros(num_units))


class AttnBlockpp(nn.Module):
    """layerspp.py:72-101 (parameter container; skip_rescale=True): the bottleneck attention block of the SGMSE-style backbone."""

    def __init__(self, channels):
        super().__init__()
        self.GroupNorm_0 = nn.GroupNorm(num_groups=min(channels // 4, 32), num_channels=channels, eps=1e-6)
        self.NIN_0, self.NIN_1, self.NIN_2, self.NIN_3 = (NIN(channels, channels) for _ in range(4))


class Combine(nn.Module):
    """layerspp.py:54-69 (parameter container, method 'sum')."""

    def __init__(self, dim1, dim2):
        super().__init__()
        self.Conv_0 = nn.Conv2d(dim1, dim2, 1)


DEFAULT_OUTPUTLAYER_KWARGS = dict(kernel_size=3, bias=False, padding="same", padding_mode="zeros")
# 3x3 convolution algorithm of the bf16 mode: direct MFMA implicit GEMM, Winograd F(2,3) wherever the shape allows it, or
# Winograd only at the low-resolution levels, or chosen per launch by grid fill ('auto'; include/flowdec_hip.h: FD_WINOGRAD*)
# Tolerances of the adaptive solvers when enhance() gets none: the reference builds `NeuralODE(node_fn, solver=solver, sensitivity=
# 'adjoint')` WITHOUT tolerances (flowdec/model.py:503-515), i.e. it runs on torchdyn's NeuralODE defaults -- atol = rtol = 1e-3 in
# torchdyn 1.0.6 (1e-4 are the adjoint's / ODEProblem's).  torchdyn is not installable offline: scripts/pin_third_party.py checks this
# value against the real package the first time it runs online (oracle/flowdec_oracle.py, section f4).
ADAPTIVE_DEFAULT_TOL = 1e-3

CONV_ALGOS = {"direct": 0, "winograd": L.FD_WINOGRAD, "winograd_lowres": L.FD_WINOGRAD_LOWRES, "auto": L.FD_WINOGRAD_AUTO,
              "latency": L.FD_LOW_LATENCY}   # one short clip on the whole chip (FD_LOW_LATENCY)


class NCSNpp(nn.Module):
    """NCSN++ vector field v(x_t, y, t) -- constructor signature of ncsnpp.py:52-75.

    Supported (every shipped FlowDec config, config/model/backbone/ncsnpp_final_no_attn.yaml, and the SGMSE-style
    ncsnpp_default_ycond.yaml): swish, BigGAN blocks, FIR [1,3,3,1], skip_rescale, progressive 'output_skip', progressive_input
    'input_skip' combined by 'sum', Fourier embedding, optionally one attention block at the bottleneck (bottleneck_attn), a
    bias-free output layer of 1x1 or 3x3 ('same' zero padding).  Attention at the resolution levels (attn_resolutions) and
    anything else raises NotImplementedError.
    """

    def __init__(self, nonlinearity="swish", nf=128, ch_mult=(1, 1, 2, 2, 2, 2, 2), num_res_blocks=2,
                 attn_resolutions=(64, 32, 16, 8), resamp_with_conv=True, conditional=True, fir=True,
                 fir_kernel=(1, 3, 3, 1), skip_rescale=True, resblock_type="biggan", progressive="output_skip",
                 progressive_input="input_skip", progressive_combine="sum", init_scale=0.0, fourier_scale=16,
                 image_size=256, embedding_type="fourier", dropout=0.0, num_channels=4,
                 output_layer_kwargs: dict = DEFAULT_OUTPUTLAYER_KWARGS, bottleneck_attn: bool = True,
                 precision: str = "bf16", conv_algo: str = "auto", side_stream: bool = True):
        super().__init__()
        self.side_stream = bool(side_stream)   # fork the time embedding / pyramid-head chain onto a second stream (FD_NO_SIDE_STREAM when False)
        ch_mult = tuple(ch_mult)
        all_res = [image_size // (2 ** i) for i in range(len(ch_mult))]
        unsupported = []
        if nonlinearity != "swish": unsupported.append("nonlinearity != swish")
        if any(r in tuple(attn_resolutions) for r in all_res): unsupported.append("attention blocks at the resolution levels (attn_resolutions)")
        if not (conditional and fir and skip_rescale and resamp_with_conv): unsupported.append("conditional/fir/skip_rescale/resamp_with_conv must be True")
        if tuple(fir_kernel) != (1, 3, 3, 1): unsupported.append("fir_kernel != [1,3,3,1]")
        if resblock_type.lower() != "biggan": unsupported.append("resblock_type != biggan")
        if progressive.lower() != "output_skip" or progressive_input.lower() != "input_skip" or progressive_combine.lower() != "sum":
            unsupported.append("progressive modes other than output_skip/input_skip/sum")
        if embedding_type.lower() != "fourier": unsupported.append("embedding_type != fourier")
        if dropout != 0.0: unsupported.append("dropout != 0 (inference only)")
        if num_channels != 4: unsupported.append("num_channels != 4")
        olk = dict(output_layer_kwargs)
        out_ks = olk.get("kernel_size", 3)
        out_ks = out_ks[0] if isinstance(out_ks, (tuple, list)) and len(set(out_ks)) == 1 else out_ks
        pad = olk.get("padding", 0)
        pad_ok = out_ks == 1 or pad == "same" or pad == 1 or (isinstance(pad, (tuple, list)) and tuple(pad) == (1, 1))
        if out_ks not in (1, 3) or olk.get("bias", True) or not pad_ok or olk.get("padding_mode", "zeros") != "zeros" or \
                any(k not in ("kernel_size", "bias", "padding", "padding_mode") for k in olk):
            unsupported.append("output layer other than a bias-free 1x1 or 3x3 ('same' zero padding) convolution")
        if unsupported:
            raise NotImplementedError("flowdec_amd.NCSNpp: unsupported configuration: " + "; ".join(unsupported))
        if precision not in ("bf16", "fp32", "mixed", "bf16x3"):
            raise ValueError("precision must be 'bf16', 'fp32', 'mixed' (f32 activations / residual stream, bf16 MFMA operands) or 'bf16x3' "
                             "(f32 storage, two-term bf16 split operands: f32-mode tolerances on the bf16 matrix cores)")
        if conv_algo not in CONV_ALGOS or (conv_algo not in ("direct", "auto") and precision != "bf16"):
            raise ValueError(f"conv_algo must be one of {sorted(CONV_ALGOS)} (precision != 'bf16': 'direct' or 'auto' only)")
        if precision in ("mixed", "bf16x3"):
            conv_algo = "direct"   # 'auto' = best available: the split / mixed operand modes have the direct kernel only
        # precision='fp32' + 'auto': 2-D Winograd F(4x4, 3x3) in exact float32 (conv_wino44f.hip) for every 3x3 layer with a multiple of 128 output
        # channels on whole 16 x 16 tiles
        self.nf, self.ch_mult, self.num_res_blocks, self.precision, self.conv_algo = nf, ch_mult, num_res_blocks, precision, conv_algo
        self.num_resolutions = len(ch_mult)
        self.bottleneck_attn, self.output_ksize = bool(bottleneck_attn), int(out_ks)
        self.output_layer = nn.Conv2d(num_channels, 2, kernel_size=self.output_ksize, padding=self.output_ksize // 2, bias=False)
        temb_dim = nf * 4
        mods = [GaussianFourierProjection(embedding_size=nf, scale=fourier_scale), nn.Linear(2 * nf, temb_dim),
                nn.Linear(temb_dim, temb_dim), nn.Conv2d(num_channels, nf, 3, padding=1)]
        hs_c, in_ch = [nf], nf
        R = self.num_resolutions
        for lvl in range(R):
            for _ in range(num_res_blocks):
                out_ch = nf * ch_mult[lvl]
                mods.append(ResnetBlockBigGANpp(in_ch, out_ch, temb_dim)); in_ch = out_ch; hs_c.append(in_ch)
            if lvl != R - 1:
                mods.append(ResnetBlockBigGANpp(in_ch, temb_dim=temb_dim, down=True))
                mods.append(Combine(num_channels, in_ch)); hs_c.append(in_ch)
        in_ch = hs_c[-1]
        mods.append(ResnetBlockBigGANpp(in_ch, temb_dim=temb_dim))
        if self.bottleneck_attn:
            mods.append(AttnBlockpp(in_ch))
        mods.append(ResnetBlockBigGANpp(in_ch, temb_dim=temb_dim))
        for lvl in reversed(range(R)):
            for _ in range(num_res_blocks + 1):
                out_ch = nf * ch_mult[lvl]
                mods.append(ResnetBlockBigGANpp(in_ch + hs_c.pop(), out_ch, temb_dim)); in_ch = out_ch
            mods.append(nn.GroupNorm(min(in_ch // 4, 32), in_ch, eps=1e-6))
            mods.append(nn.Conv2d(in_ch, num_channels, 3, padding=1))
            if lvl != 0:
                mods.append(ResnetBlockBigGANpp(in_ch, temb_dim=temb_dim, up=True))
        assert not hs_c
        self.all_modules = nn.ModuleList(mods)
        for p in self.parameters():
            p.requires_grad_(False)
        # ---- native state ----
        self._handle = None
        self._handle_sig = None
        self._ws = {}
        self._sigma_y = None
        self._stft_cfg = dict(n_fft=1534, hop=384, alpha=0.3, beta=0.33)
        self._normalize = True
        self._native_lock = threading.RLock()
        self._last_call_done = None   # event at the end of the previous native call (see _NativeCall)

    # -- native handle management ----------------------------------------------------------------
    def _config_struct(self):
        cfg = L.FdModelConfig()
        cfg.nf = self.nf
        for i, c in enumerate(self.ch_mult):
            cfg.ch_mult[i] = int(c)
        cfg.num_levels = len(self.ch_mult)
        cfg.num_res_blocks = self.num_res_blocks
        cfg.n_fft, cfg.hop = self._stft_cfg["n_fft"], self._stft_cfg["hop"]
        cfg.alpha, cfg.beta = self._stft_cfg["alpha"], self._stft_cfg["beta"]
        cfg.act_dtype = (L.FD_BF16 | CONV_ALGOS[self.conv_algo]) if self.precision == "bf16" else \
            (L.FD_F32 | {"mixed": L.FD_BF16_OPERANDS, "bf16x3": L.FD_BF16X3_OPERANDS, "fp32": CONV_ALGOS[self.conv_algo]}[self.precision])
        if not self.side_stream:
            cfg.act_dtype |= L.FD_NO_SIDE_STREAM
        return cfg

    def _arch_struct(self):
        return L.FdModelArch(int(self.bottleneck_attn), self.output_ksize)

    def invalidate(self):
        """Drop the packed device copy (called after parameters change)."""
        if self._handle is not None:
            L.load().fd_model_destroy(self._handle)
        self._handle, self._ws = None, {}

    def __del__(self):
        try:
            self.invalidate()
        except Exception:
            pass

    # copy.deepcopy / pickling (EMA copies, torch.save of the module): the native handle, its workspaces and the lock stay behind;
    # the copy repacks lazily on first use
    def __getstate__(self):
        st = self.__dict__.copy()
        st["_handle"], st["_handle_sig"], st["_ws"], st["_last_call_done"] = None, None, {}, None
        st.pop("_native_lock", None)
        return st

    def __setstate__(self, st):
        super().__setstate__(st)
        self._native_lock = threading.RLock()

    def _load_from_state_dict(self, *a, **k):
        super()._load_from_state_dict(*a, **k)
        self._handle_sig = None  # parameters changed -> repack lazily

    def _sig(self):
        p = next(self.parameters())
        sig_sigma = None if self._sigma_y is None else (self._sigma_y.data_ptr(), self._sigma_y._version)
        return (p.device, self.precision, self.conv_algo, self.side_stream, bool(self._normalize), tuple(sorted(self._stft_cfg.items())), sig_sigma,
                tuple(q._version for q in self.parameters()))

    def handle(self):
        dev = next(self.parameters()).device
        if dev.type != "cuda":
            raise RuntimeError("flowdec_amd: the model must be on the GPU (`model.cuda()`); there is no CPU path")
        sig = self._sig()
        if self._handle is not None and sig == self._handle_sig:
            return self._handle
        self.invalidate()
        lib = L.load()
        with torch.cuda.device(dev):
            h = C.c_void_p()
            cfg = self._config_struct()
            L.check(lib.fd_model_create_ex(C.byref(cfg), C.byref(self._arch_struct()), C.byref(h)))
            sd = {"backbone." + k: v for k, v in self.state_dict().items()}
            n = lib.fd_model_num_params(h)
            for i in range(n):
                name, ndim, shape = C.c_char_p(), C.c_int(), (C.c_int * 4)()
                L.check(lib.fd_model_param_info(h, i, C.byref(name), C.byref(ndim), C.byref(shape)))
                key = name.value.decode()
                if key not in sd:
                    lib.fd_model_destroy(h)
                    raise RuntimeError(f"flowdec_amd: parameter {key} missing from the module state")
                t = sd[key].detach().to("cpu", torch.float32).contiguous()
                if list(t.shape) != [shape[j] for j in range(ndim.value)]:
                    lib.fd_model_destroy(h)
                    raise RuntimeError(f"flowdec_amd: parameter {key} has shape {list(t.shape)}")
                L.check(lib.fd_model_set_param(h, name.value, C.c_void_p(t.data_ptr()), t.numel()))
            if self._sigma_y is not None:
                s = self._sigma_y.detach().to("cpu", torch.float64).contiguous().reshape(-1)
                L.check(lib.fd_model_set_sigma_y(h, C.c_void_p(s.data_ptr()), s.numel()))
            L.check(lib.fd_model_set_normalize(h, int(self._normalize)))
            L.check(lib.fd_model_finalize(h, L.stream()))
        self._handle, self._handle_sig = h, sig
        return h

    def workspace(self, key, nbytes, device):
        """One scratch buffer per call kind, grown on demand and reused (a file-by-file driver sees many clip lengths;
        keeping one buffer per (batch, length) would pin every size ever seen)."""
        kind = key[0]
        buf = self._ws.get(kind)
        if buf is None or buf.numel() < nbytes or buf.device != torch.device(device):
            self._ws.pop(kind, None)
            del buf
            check_workspace_fits(nbytes, device)
            buf = torch.empty(int(nbytes), dtype=torch.uint8, device=device)
            self._ws[kind] = buf
        return buf

    # -- reference API -----------------------------------------------------------------------------
    def forward(self, x, y, t):
        with _NativeCall(self):
            return self._forward(x, y, t)

    def _forward(self, x, y, t):
        """x, y: complex64 [B, 1, F, T]; t: [1] or [B]  ->  complex64 [B, 1, F, T] (ncsnpp.py:254-399)."""
        L.require_cuda(x, y, t)
        if x.shape != y.shape or x.ndim != 4 or x.shape[1] != 1:
            raise RuntimeError(f"NCSNpp.forward expects x, y of shape [B, 1, F, T] (got {tuple(x.shape)}, {tuple(y.shape)})")
        h = self.handle()
        lib = L.load()
        B, _, F, T = x.shape
        x = x.to(torch.complex64).contiguous(); y = y.to(torch.complex64).contiguous()
        t = t.to(torch.float32).reshape(-1).contiguous()
        out = torch.empty_like(x)
        need = lib.fd_model_workspace_bytes(h, B, T)
        if need == 0:
            raise RuntimeError("flowdec_hip: " + lib.fd_last_error().decode())
        ws = self.workspace(("fwd", B, T), need, x.device)
        with torch.cuda.device(x.device):   # L.stream() must be the stream of the tensors' device
            L.check(lib.fd_ncsnpp_forward(h, L.ptr(torch.view_as_real(x)), L.ptr(torch.view_as_real(y)), L.ptr(t), t.numel(),
                                          L.ptr(torch.view_as_real(out)), B, T, L.ptr(ws), ws.numel(), L.stream()))
        return out


class WorkspaceTooLarge(RuntimeError):
    """The workspace of a call (fd_*_workspace_bytes) exceeds the device memory that is free for it: the clip is too long for one call on
    this device."""


def check_workspace_fits(nbytes, device):
    """Raise WorkspaceTooLarge unless `nbytes` fit in the device memory free right now: free on the device plus what the caching
    allocator holds unused.  (Checked before the allocation, so that a clip that cannot fit fails with both numbers instead of an
    out-of-memory error from inside a graph capture.)"""
    dev = torch.device(device)
    if dev.type != "cuda":
        return
    free, _ = torch.cuda.mem_get_info(dev)
    avail = free + torch.cuda.memory_reserved(dev) - torch.cuda.memory_allocated(dev)
    if nbytes > avail:
        raise WorkspaceTooLarge(f"flowdec_hip: the call needs a workspace of {int(nbytes)} bytes ({nbytes / 2**30:.2f} GiB), but only "
                                f"{int(avail)} bytes ({avail / 2**30:.2f} GiB) of device memory are free on {dev}: the clip is too long "
                                f"for one call on this device")


class _NativeCall:
    """One native call at a time per model -- on the host AND on the device.  The packed model, its workspace, its I/O staging
    buffers and its hipGraph cache are shared state: (i) a lock serialises the enqueueing threads (the C ABI answers a concurrent
    call with FD_EBUSY); (ii) an event recorded at the end of every call makes the NEXT call's stream wait for it, so that two
    callers on different streams cannot overlap on the GPU inside the shared workspace.  The reference's nn.Module can be called
    from several threads / streams; this keeps that working -- calls queue up instead of failing or racing."""

    def __init__(self, backbone):
        self.bb = backbone

    def __enter__(self):
        bb = self.bb
        bb._native_lock.acquire()
        try:
            p = next(bb.parameters())
            self.stream = torch.cuda.current_stream(p.device) if p.is_cuda else None
            if self.stream is not None and bb._last_call_done is not None:
                self.stream.wait_event(bb._last_call_done)
        except BaseException:
            bb._native_lock.release()
            raise
        return self

    def __exit__(self, *exc):
        bb = self.bb
        try:
            if self.stream is not None:
                ev = torch.cuda.Event()
                ev.record(self.stream)
                bb._last_call_done = ev
        finally:
            bb._native_lock.release()
        return False


def _serialized(fn):
    import functools

    @functools.wraps(fn)
    def wrapper(self, *args, **kwargs):
        with _NativeCall(self if isinstance(self, NCSNpp) else self.backbone):
            return fn(self, *args, **kwargs)
    return wrapper


def _normfac_option(fn):
    """Adds the keyword-only option `normfac` (default None: the recording's maximum) to a long-form entry point; the call reads it as
    self._long_normfac.  The positional / keyword parameters of the entry points themselves are a pinned surface
    (tests/test_longform_cpu.py), so the option is additive here rather than one more parameter there.  Goes INSIDE @_serialized: the
    native lock is held while the value is set."""
    import functools

    @functools.wraps(fn)
    def wrapper(self, *args, normfac=None, **kwargs):
        self._long_normfac = normfac
        try:
            return fn(self, *args, **kwargs)
        finally:
            self._long_normfac = None
    return wrapper


# ------------------------------------------------------------------------------------------------
# feature extractor mirror
# ------------------------------------------------------------------------------------------------
class ComplexSTFT(nn.Module):
    """feature_extractors.py:62-109 -- torch.stft/istft replaced by the HIP DFT-GEMM kernels."""

    def __init__(self, window_fn, n_fft, sampling_rate, hop_length=None, n_hops=None, learnable_window=False):
        super().__init__()
        assert (hop_length is not None) ^ (n_hops is not None), "Exactly one of {hop_length, n_hops} must be specified!"
        if hop_length is None:
            hop_length = int(math.ceil(n_fft / n_hops))
        if window_fn != "hann" or learnable_window:
            raise NotImplementedError("flowdec_amd.ComplexSTFT: only the fixed symmetric Hann window is implemented")
        self.window = nn.Parameter(torch.signal.windows.hann(n_fft), requires_grad=False)
        self.n_fft, self.hop_length, self.sampling_rate, self.center = n_fft, hop_length, sampling_rate, True

    def forward(self, x):
        """x: [..., L] real (GPU) -> complex64 [..., n_fft/2+1, 1 + L // hop]  (feature_extractors.py:86-96)."""
        shp = x.shape
        Y, _, T = ops.stft_compress(x.reshape(-1, shp[-1]).float().contiguous(), n_fft=self.n_fft, hop=self.hop_length, alpha=1.0, beta=1.0,
                                    normalize=False)
        return Y[:, 0, :, :T].reshape(*shp[:-1], Y.shape[2], T)

    def invert(self, X, orig_length: Optional[int] = None, **kwargs):
        """torch.istft(..., length=orig_length)  (feature_extractors.py:98-109)."""
        shp = X.shape
        T = shp[-1]
        if orig_length is None:
            orig_length = self.hop_length * (T - 1)
        Xp = X.reshape(-1, 1, shp[-2], T).to(torch.complex64).contiguous()
        y = ops.decompress_istft(Xp, T, orig_length, None, n_fft=self.n_fft, hop=self.hop_length, alpha=1.0, beta=1.0)
        return y.reshape(*shp[:-2], orig_length)


class CompressAmplitudesAndScale(nn.Module):
    """feature_extractors.py:112-139.  On the hot path the arithmetic is fused into the STFT kernels; forward / invert are
    the stand-alone forms (fd_compress_spec)."""

    def __init__(self, compression_exponent: float, scale_factor: float):
        super().__init__()
        self.compression_exponent, self.scale_factor = compression_exponent, scale_factor

    def _apply_spec(self, x, inverse):
        L.require_cuda(x)
        x = x.to(torch.complex64).contiguous()
        out = torch.empty_like(x)
        with torch.cuda.device(x.device):
            L.check(L.load().fd_compress_spec(L.ptr(torch.view_as_real(x)), L.ptr(torch.view_as_real(out)), x.numel(),
                                              float(self.compression_exponent), float(self.scale_factor), int(inverse), L.stream()))
        return out

    def forward(self, x):
        return self._apply_spec(x, False)

    def invert(self, x):
        return self._apply_spec(x, True)


class AmplitudeCompressedComplexSTFT(nn.Module):
    """feature_extractors.py:29-59."""

    def __init__(self, window_fn, n_fft, sampling_rate, alpha, beta, hop_length=None, n_hops=None, learnable_window=False):
        super().__init__()
        self.complex_stft = ComplexSTFT(window_fn, n_fft, sampling_rate, hop_length=hop_length, n_hops=n_hops,
                                        learnable_window=learnable_window)
        self.compress = CompressAmplitudesAndScale(alpha, beta)

    def _cfg(self):
        return dict(n_fft=self.complex_stft.n_fft, hop=self.complex_stft.hop_length,
                    alpha=float(self.compress.compression_exponent), beta=float(self.compress.scale_factor))

    def forward(self, x, **kwargs):
        """x: [B, C, T] or [B, T] real (GPU) -> complex STFT, compressed (no normalisation, no padding)."""
        shp = x.shape
        Y, _, T = ops.stft_compress(x.reshape(-1, shp[-1]).float().contiguous(), normalize=False, **self._cfg())
        return Y[:, 0, :, :T].reshape(*shp[:-1], Y.shape[2], T)

    def invert(self, X, orig_length: Optional[int] = None, **kwargs):
        shp = X.shape
        T = shp[-1]
        if orig_length is None:
            orig_length = self.complex_stft.hop_length * (T - 1)
        Xp = X.reshape(-1, 1, shp[-2], T).to(torch.complex64).contiguous()
        y = ops.decompress_istft(Xp, T, orig_length, None, **self._cfg())
        return y.reshape(*shp[:-2], orig_length)


# ------------------------------------------------------------------------------------------------
# the staging base of the three model classes
# ------------------------------------------------------------------------------------------------
def sigma_y_from_file(filename: str, factor: float = 1.0, kernel_bandwidth: Optional[float] = None) -> torch.Tensor:
    """flowdec/data/sigma_models/__init__.py:21-47 (gaussian_filter(mode='nearest') restated in NumPy)."""
    if not os.path.isabs(filename):
        filename = os.path.join(_DATA, os.path.basename(filename))
    curve = np.load(filename).astype(np.float64)
    if kernel_bandwidth is not None:
        radius = int(4.0 * float(kernel_bandwidth) + 0.5)
        k = np.arange(-radius, radius + 1, dtype=np.float64)
        w = np.exp(-0.5 * (k / kernel_bandwidth) ** 2); w /= w.sum()
        xp = np.concatenate([np.full(radius, curve[0]), curve, np.full(radius, curve[-1])])
        curve = np.correlate(xp, w, mode="valid")
    return factor * torch.from_numpy(curve).unsqueeze(-1)


def _check_step_control(step_control, solver, who):
    """`step_control` of the adaptive solvers: None / 'batch' (one controller for the batch) or 'clip' (one per clip) -> per-clip?"""
    if step_control not in (None, "batch", "clip"):
        raise ValueError(f"{who}: step_control must be None, 'batch' or 'clip' (got {step_control!r})")
    if step_control is not None and solver not in L.ADAPTIVE_SOLVERS:
        raise ValueError(f"{who}: step_control={step_control!r} belongs to the adaptive solvers {sorted(L.ADAPTIVE_SOLVERS)}; "
                         f"the fixed-step solver {solver!r} has no step size to control")
    return step_control == "clip"


def _per_clip_generators(generator, noise, B):
    """One generator per clip from `generator` (one for all clips, drawn clip by clip, or a list of one per clip); checks the counts."""
    gens = generator if isinstance(generator, (list, tuple)) else [generator] * B
    if noise is not None and len(noise) != B or len(gens) != B:
        raise RuntimeError("enhance_batch: one noise tensor / generator per clip")
    return gens


def _preprocess_info(Lw, normfac, T, squeeze_dims):
    """preprocess_info of the reference (model.py:161-162); normfac: the B factors of the clips, T: the frames before pad_spec."""
    return dict(orig_length=Lw, normfac=normfac.reshape(-1, 1, 1), undo_pad_fn=(lambda Y_, T=T: Y_[..., :T]), squeeze_dims=squeeze_dims)


def _traj_waveforms(traj, T, Lw, normfac, cfg, lengths=None):
    """Every state of a solver trajectory [N + 1, B, 1, F, T_pad] back in the time domain -> list of N + 1 waveforms [B, 1, Lw]."""
    return [ops.decompress_istft(X, T, Lw, normfac, lengths=lengths, **cfg).reshape(-1, 1, Lw) for X in traj]


def _preprocess(model, y, x=None, comp_eps=None):
    """EnhancementModel._preprocess (model.py:129-163): [L] / [1, L] / [B, 1, L] waveform(s) -> the reference's 3-tuple
    (Y, X, preprocess_info): Y [B, 1, F, T_pad] complex64 with the frame axis zero-padded to a multiple of 64, X the same
    features of the optional clean waveform `x` normalised by y's factor (None when x is None)."""
    if comp_eps is not None:
        raise NotImplementedError("flowdec_amd: comp_eps (a training-time regulariser, feature_extractors.py:124-125) is not supported")
    if x is not None and x.shape != y.shape:
        raise RuntimeError(f"x and y must have the same shape (got {tuple(x.shape)} vs {tuple(y.shape)})")   # model.py:141
    dev = model.device
    y, squeeze_dims = _to_3d(y, "expected")
    B, Lw = y.shape[0], y.shape[-1]
    cfg = model.feature_extractor._cfg()
    with torch.cuda.device(dev):
        Y, normfac, T = ops.stft_compress(y.reshape(B, Lw).to(dev, torch.float32).contiguous(), normalize=model.normalize_mode == "noisy", **cfg)
        X = None
        if x is not None:   # x / normfac(y) (util/other.py:79-81), then the same feature extractor and padding, without a second normalisation
            xn = x.reshape(B, Lw).to(dev, torch.float32) / normfac.reshape(B, 1)
            X, _, _ = ops.stft_compress(xn.contiguous(), normalize=False, **cfg)
    return Y, X, _preprocess_info(Lw, normfac, T, squeeze_dims)


def _postprocess(model, X_hat, preprocess_info, inv_kwargs=None, batch_filter=None):
    """EnhancementModel._postprocess (model.py:165-190): undo padding, invert the features, [select batch items,] restore the
    level and the rank.  `inv_kwargs` is forwarded to the feature extractor's invert like the reference does; the native
    inverse has no optional arguments, so a non-empty dict is rejected instead of being silently ignored."""
    I = preprocess_info
    assert {"orig_length", "normfac", "undo_pad_fn", "squeeze_dims"} <= I.keys()   # model.py:180
    if inv_kwargs:
        raise NotImplementedError(f"flowdec_amd: feature_extractor.invert takes no extra arguments (got {sorted(inv_kwargs)})")
    T = I["undo_pad_fn"](X_hat).shape[-1]   # frames before pad_spec
    Lw = I["orig_length"]
    B = X_hat.shape[0]
    Xp = X_hat.to(torch.complex64).contiguous()             # the kernel reads the first T frames of the (padded) frame axis
    normfac = I["normfac"]   # [B, 1, 1] tensor ('noisy') or the float 1.0 of normalize_mode='none' (util/other.py:70)
    normfac = normfac.reshape(-1).float() if torch.is_tensor(normfac) else torch.full((1,), float(normfac))
    normfac = normfac.expand(B) if normfac.numel() == 1 else normfac
    with torch.cuda.device(Xp.device):
        x_hat = ops.decompress_istft(Xp, T, Lw, normfac.to(Xp.device).contiguous(), **model.feature_extractor._cfg())
    x_hat = x_hat.reshape(B, 1, Lw)
    if batch_filter is not None:   # model.py:185-187 (x * normfac commutes with selecting batch items)
        x_hat = x_hat[torch.as_tensor(batch_filter, device=x_hat.device)]
    for _ in range(I["squeeze_dims"]):
        x_hat = x_hat.squeeze(0)
    return x_hat


class _WaveModel(nn.Module):
    """What FlowModel, ScoreModel and RegressionModel share: the reference's waveform plumbing (EnhancementModel._preprocess /
    _postprocess, model.py:129-190) and the staging of every native enhance call -- resident device buffers, the capture-safe side
    stream, the equal-length call (`_wave_call`) and the ragged call (`_ragged_call`).  A model class adds its argument checks and a
    `launch` closure around its own native entry point."""
    strict_loading = False

    def __init__(self, backbone: NCSNpp, feature_extractor: AmplitudeCompressedComplexSTFT, sampling_rate: int = 48000,
                 lr: float = 1e-4, normalize_mode: str = "noisy", **kwargs):
        super().__init__()
        assert normalize_mode in ("noisy", "none")
        self.sampling_rate, self.normalize_mode, self.lr = sampling_rate, normalize_mode, lr
        self.backbone, self.feature_extractor = backbone, feature_extractor
        self._io, self._side_stream = {}, None

    # EnhancementModel._preprocess / _postprocess (model.py:129-190) as stand-alone calls
    def _preprocess(self, y, x=None, comp_eps=None):
        return _preprocess(self, y, x, comp_eps)

    def _postprocess(self, X_hat, preprocess_info, inv_kwargs=None, batch_filter=None):
        return _postprocess(self, X_hat, preprocess_info, inv_kwargs, batch_filter)

    @property
    def device(self):
        return next(self.backbone.parameters()).device

    def load_state_dict(self, state_dict, strict: bool = False, **kw):
        # the reference sets strict_loading = False (model.py:397)
        return super().load_state_dict(state_dict, strict=strict, **kw)

    def _sync_native(self):
        self.backbone._sigma_y = getattr(self, "sigma_y", None)   # the flow model's; the baselines have none
        self.backbone._stft_cfg = self.feature_extractor._cfg()
        self.backbone._normalize = self.normalize_mode == "noisy"
        return self.backbone.handle()

    def _native_call(self):
        """The `_NativeCall` of this model's backbone, for native calls made outside this module (flowdec_amd/loss.py)."""
        return _NativeCall(self.backbone)

    def _gpu(self):
        dev = self.device
        if dev.type != "cuda":
            raise RuntimeError("flowdec_amd: move the model to the GPU first (`model.cuda()`)")
        return dev

    def _frames(self, Lw):
        """-> (F, T, T_pad) of a clip of Lw samples."""
        lib, cfg = L.load(), self.feature_extractor._cfg()
        T = lib.fd_num_frames(Lw, cfg["hop"])
        return cfg["n_fft"] // 2 + 1, T, lib.fd_padded_frames(T)

    @contextlib.contextmanager
    def _on_side_stream(self, dev):
        """Stream capture is illegal on the legacy default stream: the native calls run on a side stream that is ordered after / before
        the caller's current stream (yielded, for the `record_stream` of what the caller gets back)."""
        cur = torch.cuda.current_stream(dev)
        if self._side_stream is None:
            self._side_stream = torch.cuda.Stream(dev)
        side = self._side_stream
        side.wait_stream(cur)
        with torch.cuda.stream(side):
            yield cur
        cur.wait_stream(side)

    def _io_entry(self, B, Lw, dev, n_draws=0, seeded=False, ragged=False):
        """The resident device buffers of the enhance calls: ONE shape (rows, row length, device) per model.  A captured graph is keyed on
        their addresses, so y and out live as long as the shape does, lens and seeds come with the first call that needs them and stay,
        and noise [n_draws, B, 1, F, T_pad] lives until n_draws changes -- to 0 (a seeded call, or a model without noise): to None, so
        a seeded call holds no noise plane."""
        key = (B, Lw, str(dev))
        io = self._io.get(key)
        if io is None:
            io = dict(y=torch.empty(B, Lw, dtype=torch.float32, device=dev), out=torch.empty(B, Lw, dtype=torch.float32, device=dev),
                      lens=None, seeds=None, noise=None)
            self._io = {key: io}
        if ragged and io["lens"] is None:
            io["lens"] = torch.empty(B, dtype=torch.int32, device=dev)
        if seeded and io["seeds"] is None:
            io["seeds"] = torch.empty(B, dtype=torch.int64, device=dev)
        if n_draws != (0 if io["noise"] is None else io["noise"].shape[0]):
            F, _, Tp = self._frames(Lw)
            io["noise"] = None   # (released before its successor is allocated)
            if n_draws:
                io["noise"] = torch.empty(n_draws, B, 1, F, Tp, dtype=torch.complex64, device=dev)
        return io

    def _enhance_workspace(self, lib, h, B, Lw, dev):
        need = lib.fd_enhance_workspace_bytes(h, B, Lw)
        if need == 0:
            raise RuntimeError("flowdec_hip: " + lib.fd_last_error().decode())
        return self.backbone.workspace(("enh", B, Lw), need, dev)

    @_serialized
    def _wave_call(self, y, n_draws, noise, generator, launch, return_preprocess_info=False, seed=None, return_traj=False):
        """The staging of `enhance`: y [L] / [1, L] / [B, 1, L] into the resident buffers, then launch(lib, h, io, B, L, ws) on the side
        stream; io = dict(y [B, L], out [B, L], noise [n_draws, B, 1, F, Tp], seeds int64 [B], ...).  With `seed` the seeds are filled and
        no noise tensor is (a member the call does not fill is None or stale).  launch returns None -- the result is io["out"], its
        normfac where fd_enhance's front end left it in ws -- or its own (x_hat [B, 1, L], normfac [B]); with return_traj the pair
        (trajectory, list of waveforms [B, 1, L]), which is returned on the model's device like the reference does."""
        dev = self._gpu()
        orig_device = y.device
        y3, squeeze_dims = _to_3d(y, "enhance expects")
        lib = L.load()
        h = self._sync_native()
        B, Lw = y3.shape[0], y3.shape[-1]
        with torch.cuda.device(dev):
            io = self._io_entry(B, Lw, dev, 0 if seed is not None else n_draws, seeded=seed is not None)
            io["y"].copy_(y3.reshape(B, Lw))
            if seed is not None:
                io["seeds"].copy_(fd_noise.seeds_to_tensor(seed, B, dev))
            elif n_draws:
                if noise is not None:
                    io["noise"].copy_(noise.to(dev, torch.complex64).reshape(io["noise"].shape))
                else:
                    io["noise"].copy_(torch.randn(io["noise"].shape, dtype=torch.complex64, device=dev, generator=generator))
            ws = self._enhance_workspace(lib, h, B, Lw, dev)
            with self._on_side_stream(dev) as cur:
                res = launch(lib, h, io, B, Lw, ws)
                if res is None:
                    res = io["out"].reshape(B, 1, Lw).clone(), None
                    if return_preprocess_info:
                        off = lib.fd_enhance_normfac_offset(h, B, Lw)
                        res = res[0], ws[off:off + 4 * B].view(torch.float32).clone()
        first, second = res
        first.record_stream(cur)
        if return_traj:
            for w in second:
                w.record_stream(cur)
            return first, [w.reshape(w.shape[squeeze_dims:]) for w in second]
        x_hat = first.reshape(first.shape[squeeze_dims:]).to(orig_device)
        return (x_hat, _preprocess_info(Lw, second, self._frames(Lw)[1], squeeze_dims)) if return_preprocess_info else x_hat

    @_serialized
    def _ragged_call(self, clips, n_draws, noise, generator, seeds, launch):
        """The staging of `enhance_batch`: clips of ONE T_pad bucket as zero-padded rows of a [B, hop * T_pad - 1] buffer, then
        launch(lib, h, io, B, Lrow, ws) on the side stream; io as in `_wave_call` plus lens int32 [B].  Clip b's planes are noise[b]
        ([n_draws, 1, 1, F, Tp]) or one draw of that shape from its generator -- what `_wave_call` draws for the clip alone; with `seeds`
        no noise tensor is filled.  launch returns None (the rows are io["out"]) or its own rows [B, Lrow].  -> list of waveforms, each
        with the shape and on the device of its clip."""
        dev = self._gpu()
        clips = list(clips)
        if not clips:
            return []
        lib = L.load()
        h = self._sync_native()
        flat, lens, Tp, Lrow = _ragged_bucket(clips, self.feature_extractor._cfg())
        B = len(flat)
        gens = _per_clip_generators(generator, noise, B)
        with torch.cuda.device(dev):
            if seeds is not None:
                n_draws = 0
            io = self._io_entry(B, Lrow, dev, n_draws, seeded=seeds is not None, ragged=True)
            io["lens"].copy_(padded_rows(flat, Lrow, dev, out=io["y"])[1])
            for b in range(B if n_draws else 0):
                shape = (n_draws, 1, 1) + tuple(io["noise"].shape[3:])
                z = noise[b].to(dev, torch.complex64).reshape(shape) if noise is not None else \
                    torch.randn(shape, dtype=torch.complex64, device=dev, generator=gens[b])
                io["noise"][:, b:b + 1].copy_(z)
            if seeds is not None:
                io["seeds"].copy_(fd_noise.seeds_to_tensor(list(seeds) if not isinstance(seeds, torch.Tensor) else seeds, B, dev))
            ws = self._enhance_workspace(lib, h, B, Lrow, dev)
            with self._on_side_stream(dev) as cur:
                rows = launch(lib, h, io, B, Lrow, ws)
                rows = io["out"] if rows is None else rows
                outs = [rows[b, :lens[b]].clone() for b in range(B)]
        res = []
        for b, c in enumerate(clips):
            outs[b].record_stream(cur)
            res.append(outs[b].reshape(c.shape).to(c.device))
        return res

    # -- long-form: a recording of any length as overlapping rows of one bucket (flowdec_amd/longform.py; include/flowdec_hip.h "Long-form").
    # The machinery is the same for the three classes; a class adds `_chunks_call`, the hook around its native chunks entry point.  The
    # streaming pools (flowdec_amd/stream.py) issue the same hook between fd_stream_gather and fd_stream_emit.
    _draws_noise = True   # RegressionModel: False -- it takes no seed, and its rows no frame0

    def _chunks_call(self, who: str = "enhance_long", **sampler):
        """The long-form hook: checks the class's sampler arguments (the refusals need no GPU) and returns
        call(lib, h, y, lens, seeds, frame0, normfac, out, B, Lrow, ws, use_graph), which issues the class's native chunks call on the
        current stream -- y / out [B, Lrow] float32, lens int32 [B], seeds uint64 [B], frame0 int32 [B], normfac float32 [B] or None:
        device pointers (ctypes), ws the workspace tensor.  All rows of a call share the one sampler configuration."""
        raise NotImplementedError(f"{type(self).__name__} has no long-form entry point")

    def _long_buffers(self, B, Lrow, dev):
        """The device arrays of the long-form native calls.  They live as long as the shape does: a captured graph is keyed on their
        addresses, so every group of rows of every file of that shape replays one graph.  Not an entry of `_io`: a caller that alternates
        `enhance` and `enhance_long` keeps both shapes, and both graphs, resident."""
        key = (B, Lrow, str(dev))
        if getattr(self, "_io_long_key", None) != key:
            self._io_long = dict(y=torch.zeros(B, Lrow, dtype=torch.float32, device=dev), out=torch.empty(B, Lrow, dtype=torch.float32, device=dev),
                                 lens=torch.empty(B, dtype=torch.int32, device=dev), seeds=torch.empty(B, dtype=torch.int64, device=dev),
                                 frame0=torch.empty(B, dtype=torch.int32, device=dev), normfac=torch.empty(B, dtype=torch.float32, device=dev))
            self._io_long_key = key
        return self._io_long

    @torch.no_grad()
    @_serialized
    def _enhance_long(self, y, call, seed=None, row_frames: int = 3712, halo_frames: int = 256, xfade: Optional[int] = None,
                      rows_per_call: int = 8, use_graph: bool = True, normfac=None):
        """`FlowModel.enhance_long` for any of the three classes: `call` = self._chunks_call(<the class's sampler arguments>).  y, seed (a
        model that draws no noise ignores it), the geometry and `normfac` as documented there.  A recording of one row equals the class's
        `enhance(y, seed=seed)` bit for bit, a longer one is the float32 stitch of its rows, and the result depends neither on
        `rows_per_call` nor on graph or eager execution."""
        if not self._draws_noise:
            seed = 0
        elif seed is None:
            seed = int(torch.randint(0, 2 ** 63 - 1, (1,)).item())
        plan = self._long_plan(y, seed, row_frames, halo_frames, xfade, rows_per_call, normfac)
        with self._long_stream(plan) as (lib, h, y_dev):
            row_out = self._long_run_jobs(lib, h, plan, y_dev, plan.jobs, call, rows_per_call, use_graph)
            x_hat = self._long_stitch_rows(lib, plan, row_out)
        x_hat.record_stream(torch.cuda.current_stream(plan.dev))
        return x_hat.reshape(y.shape).to(y.device)

    @torch.no_grad()
    @_serialized
    def _enhance_long_rows(self, y, call, jobs: Optional[Tuple[int, int]] = None, seed=None, row_frames: int = 3712, halo_frames: int = 256,
                           xfade: Optional[int] = None, rows_per_call: int = 8, use_graph: bool = True, normfac=None):
        """`FlowModel.enhance_long_rows` for any of the three classes (`call` as in `_enhance_long`)."""
        if not self._draws_noise:
            seed = 0
        elif seed is None:
            raise ValueError("enhance_long_rows: pass the recording's seed (the calls that share a recording must share it)")
        plan = self._long_plan(y, seed, row_frames, halo_frames, xfade, rows_per_call, normfac)
        lo, hi = (0, len(plan.jobs)) if jobs is None else (int(jobs[0]), int(jobs[1]))
        if not 0 <= lo <= hi <= len(plan.jobs):
            raise ValueError(f"enhance_long_rows: jobs {(lo, hi)} outside the recording's {len(plan.jobs)} (channel, row) jobs")
        with self._long_stream(plan) as (lib, h, y_dev):
            row_out = self._long_run_jobs(lib, h, plan, y_dev, plan.jobs[lo:hi], call, rows_per_call, use_graph)
        row_out.record_stream(torch.cuda.current_stream(plan.dev))
        return row_out

    @torch.no_grad()
    @_serialized
    def _enhance_long_stitch(self, y, row_out, row_frames: int = 3712, halo_frames: int = 256, xfade: Optional[int] = None):
        plan = self._long_plan(y, 0, row_frames, halo_frames, xfade, 1)
        if tuple(row_out.shape) != (len(plan.jobs), plan.Lrow) or row_out.dtype != torch.float32:
            raise ValueError(f"enhance_long_stitch: expected float32 row outputs {(len(plan.jobs), plan.Lrow)} (got {row_out.dtype} {tuple(row_out.shape)})")
        row_out = row_out.to(plan.dev).contiguous()
        with self._long_stream(plan, upload=False) as (lib, h, _):
            x_hat = self._long_stitch_rows(lib, plan, row_out)
        x_hat.record_stream(torch.cuda.current_stream(plan.dev))
        return x_hat.reshape(y.shape).to(y.device)

    def _enhance_long_jobs(self, y, row_frames: int = 3712, halo_frames: int = 256, xfade: Optional[int] = None) -> int:
        return len(self._long_plan(y, 0, row_frames, halo_frames, xfade, 1).jobs)

    def _long_plan(self, y, seed, row_frames, halo_frames, xfade, rows_per_call, normfac=None):
        """Argument checks and the host-side geometry of a long-form call: rows, bucket, the (channel, row) job pool, per-channel seeds."""
        from types import SimpleNamespace
        if int(rows_per_call) < 1:
            raise ValueError(f"enhance_long: rows_per_call must be >= 1 (got {rows_per_call})")
        dev = self._gpu()
        y3, _ = _to_3d(y, "enhance_long expects", rows="C")
        lib = L.load()
        cfg = self.feature_extractor._cfg()
        hop = cfg["hop"]
        C_, n = y3.shape[0], y3.shape[-1]
        rows = longform.plan_rows(n, hop, row_frames, halo_frames, xfade)
        xfade = 2 * hop if xfade is None else int(xfade)
        Tp = int(lib.fd_padded_frames(lib.fd_num_frames(rows[0].length, hop)))
        Lrow = hop * Tp - 1
        ops.check_ragged_lengths([r.length for r in rows], Lrow, cfg["n_fft"], hop)
        if n // hop + Tp >= 2 ** 31:
            raise RuntimeError(f"enhance_long: {n} samples exceed the 2^31 absolute frames of the noise contract")
        normalize = self.normalize_mode == "noisy"
        if normfac is not None:
            if not normalize:
                raise ValueError("enhance_long: normfac needs normalize_mode='noisy' (a 'none' model does not normalise)")
            if isinstance(normfac, str):
                if normfac != "causal":
                    raise ValueError(f"enhance_long: normfac is None, a float, a per-channel tensor or 'causal' (got {normfac!r})")
            else:
                normfac = torch.as_tensor(normfac, dtype=torch.float32).reshape(-1)
                if normfac.numel() not in (1, C_) or not bool((torch.isfinite(normfac) & (normfac > 0)).all()):
                    raise ValueError(f"enhance_long: normfac must be one positive finite factor, or one per channel ({C_})")
                normfac = normfac.expand(C_)
        jobs = [(c, r) for c in range(C_) for r in rows]          # every channel's rows, one pool: a row's result depends on nothing else
        return SimpleNamespace(dev=dev, y3=y3, C=C_, n=n, rows=rows, R=len(rows), xfade=xfade, Tp=Tp, Lrow=Lrow, jobs=jobs,
                               file_seeds=fd_noise.seeds_to_tensor(seed, C_, "cpu").tolist(), normalize=normalize, normfac=normfac)

    @contextlib.contextmanager
    def _long_stream(self, plan, upload: bool = True):
        """The long-form native calls run on the side stream, after the upload of the recording.  -> (lib, handle, the recording [C, n] on
        the device, or None without `upload`)."""
        lib = L.load()
        h = self._sync_native()
        with torch.cuda.device(plan.dev):
            y_dev = plan.y3.reshape(plan.C, plan.n).to(plan.dev, torch.float32).contiguous() if upload else None
            with self._on_side_stream(plan.dev):
                yield lib, h, y_dev

    def _long_run_jobs(self, lib, h, plan, y_dev, jobs, call, rows_per_call, use_graph):
        """`jobs` (a slice of plan.jobs) through the class's chunks call in balanced groups of at most `rows_per_call` -> [len(jobs), Lrow]."""
        dev, Lrow, normalize = plan.dev, plan.Lrow, plan.normalize
        row_out = torch.empty(len(jobs), Lrow, dtype=torch.float32, device=dev)
        if not jobs:
            return row_out
        n_calls = -(-len(jobs) // int(rows_per_call))
        B = -(-len(jobs) // n_calls)                              # balanced groups: at most n_calls - 1 filler rows
        io = self._long_buffers(B, Lrow, dev)
        file_normfac = row_index = None                           # [C], or [C, R] with normfac="causal"
        if normalize and plan.normfac is None:                    # the WHOLE recording's factor, whichever of its jobs run here
            file_normfac = torch.empty(plan.C, dtype=torch.float32, device=dev)
            L.check(lib.fd_normfac(L.ptr(y_dev), None, plan.C, plan.n, L.ptr(file_normfac), L.stream()))
        elif normalize and isinstance(plan.normfac, str):         # "causal": the peak of [0, row end) -- one prefix pass per row that runs here
            file_normfac = torch.ones(plan.C, plan.R, dtype=torch.float32, device=dev)
            row_index = {r.start: j for j, r in enumerate(plan.rows)}
            for c, r in sorted(set((c, r) for c, r in jobs)):
                L.check(lib.fd_normfac(L.ptr(y_dev[c]), None, 1, r.start + r.length, L.ptr(file_normfac[c, row_index[r.start]:]), L.stream()))
            file_normfac = file_normfac.reshape(-1)
        elif normalize:
            file_normfac = plan.normfac.to(dev)
        ws = self._enhance_workspace(lib, h, B, Lrow, dev)
        for g0 in range(0, len(jobs), B):
            group = jobs[g0:g0 + B]
            group = group + [group[-1]] * (B - len(group))    # filler rows keep (B, T_pad) -- and the graph -- fixed; their output is dropped
            for b, (c, r) in enumerate(group):
                io["y"][b, :r.length].copy_(y_dev[c, r.start:r.start + r.length])
                io["y"][b, r.length:].zero_()
            chans = torch.tensor([c if row_index is None else c * plan.R + row_index[r.start] for c, r in group], dtype=torch.int64)
            io["lens"].copy_(torch.tensor([r.length for _, r in group], dtype=torch.int32))
            io["frame0"].copy_(torch.tensor([r.frame0 for _, r in group], dtype=torch.int32))
            io["seeds"].copy_(torch.tensor([plan.file_seeds[c] for c, _ in group], dtype=torch.int64))
            if normalize:
                io["normfac"].copy_(file_normfac[chans.to(dev)])
            call(lib, h, L.ptr(io["y"]), L.ptr(io["lens"]), L.ptr(io["seeds"]), L.ptr(io["frame0"]), L.ptr(io["normfac"]) if normalize else None,
                 L.ptr(io["out"]), B, Lrow, ws, use_graph)
            k = min(B, len(jobs) - g0)
            row_out[g0:g0 + k].copy_(io["out"][:k])
        return row_out

    def _long_stitch_rows(self, lib, plan, row_out):
        """fd_stitch_chunks per channel over the outputs of all jobs -> [C, n]."""
        dev, rows, R, n, xfade = plan.dev, plan.rows, plan.R, plan.n, plan.xfade
        x_hat = torch.empty(plan.C, n, dtype=torch.float32, device=dev)
        starts = torch.tensor([r.start for r in rows], dtype=torch.int32).to(dev)
        bounds = torch.tensor([r.xfade_lo for r in rows[1:]], dtype=torch.int32).to(dev) if R > 1 else None
        weights = torch.from_numpy(longform.stitch_weights(xfade)).to(dev) if R > 1 and xfade > 0 else None
        for c in range(plan.C):
            L.check(lib.fd_stitch_chunks(L.ptr(row_out[c * R:(c + 1) * R]), plan.Lrow, L.ptr(starts), L.ptr(bounds), R, L.ptr(weights),
                                         xfade if R > 1 else 0, L.ptr(x_hat[c]), n, L.stream()))
        return x_hat


# ------------------------------------------------------------------------------------------------
# FlowModel
# ------------------------------------------------------------------------------------------------
class FlowModel(_WaveModel):
    """Drop-in for flowdec.model.FlowModel on the inference path (model.py:391-536).

    Extensions over the reference signature: ``enhance(..., noise=None, generator=None)`` to inject /
    seed the initial Gaussian noise (the reference draws it from the global device RNG, model.py:512),
    ``seed=`` (the library's own counter-based noise, generated on the GPU from one 64-bit seed per clip: an int -- clip b
    uses ``flowdec_amd.noise.clip_seed(seed, b)`` --, B ints or an int64 / uint64 tensor [B]; no noise tensor is filled),
    and ``use_graph`` (hipGraph replay of the whole solve).  ``with_grad=True`` is not supported.
    """

    def __init__(self, backbone: NCSNpp, feature_extractor: AmplitudeCompressedComplexSTFT, sampling_rate: int,
                 sigma_x=0.0, sigma_y=0.66, flow_matcher=None, lr: float = 1e-4, normalize_mode: str = "noisy", **kwargs):
        super().__init__(backbone, feature_extractor, sampling_rate, lr=lr, normalize_mode=normalize_mode)
        self.flow_matcher = flow_matcher
        if callable(sigma_x) and not isinstance(sigma_x, torch.Tensor):   # model.py:408-413: kept as given; only `valid_loss` reads sigma_x, and refuses it
            self.sigma_x = sigma_x
        else:
            self.sigma_x = nn.Parameter(sigma_x if isinstance(sigma_x, torch.Tensor) else torch.tensor(float(sigma_x)), requires_grad=False)
        self.error_weighting = kwargs.get("error_weighting")
        self.sigma_y = nn.Parameter(sigma_y if isinstance(sigma_y, torch.Tensor) else torch.tensor(float(sigma_y)), requires_grad=False)

    def forward(self, xt, y, t):
        if t.ndim == 0:
            t = t.unsqueeze(0)  # model.py:471-472
        self._sync_native()
        return self.backbone(xt, y, t)

    @torch.no_grad()
    def enhance(self, y, return_preprocess_info: bool = False, N: int = 50, solver: str = "euler", with_grad: bool = False,
                sigma_fac: float = 1.0, return_traj: bool = False, noise=None, generator=None, use_graph: bool = True, seed=None,
                step_control: Optional[str] = None, **kwargs):
        """Enhances a coded/noisy waveform y (model.py:476-528).  y: [L], [1, L] or [B, 1, L].

        The adaptive solvers ('dopri5', 'tsit5'; `atol=`, `rtol=`) take `step_control`: None / 'batch' accepts or rejects a step on ONE
        error ratio over the whole batch (torchdyn's behaviour for a batched call), so a clip's result depends on its batch companions;
        'clip' gives every clip its own controller -- clip b is bit-identical to the one-clip call on it, alone, in any batch and in any
        shard of a batch, and `seed=` draws the noise inside the solver (no noise tensor).  `last_nfe` is then the largest per-clip
        NFE; `last_nfe_per_clip`, `last_rejected_per_clip` ([B] int tensors) and `last_evals` (evaluations of the whole batch that ran:
        clips that are done ride along until the slowest one is) give the detail."""
        fd_noise.exclusive(seed=seed, noise=noise, generator=generator)
        if with_grad:
            raise NotImplementedError("flowdec_amd.FlowModel.enhance: with_grad=True (backprop through the solver) is out of scope")
        adaptive = solver in L.ADAPTIVE_SOLVERS
        if not adaptive and solver not in L.SOLVERS:
            raise ValueError(f"unknown solver {solver!r}; supported: {sorted(L.SOLVERS) + sorted(L.ADAPTIVE_SOLVERS)}")
        per_clip = _check_step_control(step_control, solver, "enhance")
        atol, rtol = float(kwargs.get("atol", ADAPTIVE_DEFAULT_TOL)), float(kwargs.get("rtol", ADAPTIVE_DEFAULT_TOL))

        def launch(lib, h, io, B, Lw, ws):
            z, seeds = (io["noise"], None) if seed is None else (None, io["seeds"])
            if adaptive:
                if seeds is not None and not per_clip:   # the batch-global driver only needs the initial plane: filled by the library, then the unseeded call
                    z, seeds = fd_noise.noise_fill(seeds, *self._frames(Lw)[::2]), None
                return self._enhance_adaptive(lib, h, io["y"], z, seeds, B, Lw, N, sigma_fac, return_traj, atol, rtol, L.ADAPTIVE_SOLVERS[solver], per_clip)
            if return_traj:
                return self._enhance_traj(lib, h, io["y"], z, seeds, B, Lw, N, solver, sigma_fac)
            if seeds is not None:
                L.check(lib.fd_enhance_seeded(h, L.ptr(io["y"]), None, L.ptr(seeds), float(sigma_fac), int(N),
                                              L.SOLVERS[solver], L.ptr(io["out"]), B, Lw, L.ptr(ws), ws.numel(), int(use_graph), L.stream()))
            else:
                L.check(lib.fd_enhance(h, L.ptr(io["y"]), L.ptr(torch.view_as_real(z)), float(sigma_fac), int(N),
                                       L.SOLVERS[solver], L.ptr(io["out"]), B, Lw, L.ptr(ws), ws.numel(), int(use_graph), L.stream()))
        return self._wave_call(y, 1, noise, generator, launch, return_preprocess_info, seed=seed, return_traj=return_traj)

    @torch.no_grad()
    def enhance_batch(self, clips, N: int = 50, solver: str = "euler", sigma_fac: float = 1.0, noise=None, generator=None,
                      use_graph: bool = True, seeds=None, step_control: Optional[str] = None, atol: float = ADAPTIVE_DEFAULT_TOL,
                      rtol: float = ADAPTIVE_DEFAULT_TOL):
        """`[self.enhance(c, N=N, solver=solver) for c in clips]` as ONE native call (fd_enhance_ragged) for clips of DIFFERENT
        lengths whose spectrograms pad to the same T_pad -- what the reference's driver does file by file (enhance.py:96-137).

        clips: sequence of waveforms [L_i], [1, L_i] or [1, 1, L_i].  Returns a list of tensors, each with the shape and on the
        device of its input.  Every clip's result is BIT-IDENTICAL to `self.enhance(clip)` with the same noise: per-clip
        normalisation, reflect padding, frame count, zero padding of the frame axis, iSTFT length (model.py:129-190); the network
        itself never mixes batch items.  Initial noise: `noise` = one [1, 1, F, T_pad] complex tensor per clip, or `generator` =
        one torch.Generator (drawn clip by clip, i.e. the stream a one-by-one loop would consume) or a list of one per clip, or
        `seeds` = one 64-bit seed per clip (a sequence or an int64 / uint64 tensor) for the library's own noise: clip i then equals
        `self.enhance(clip_i, seed=[seeds[i]])`.

        The adaptive solvers ('dopri5', 'tsit5', with `atol`, `rtol`) run here with step_control='clip' only: every clip then steps under
        its own controller and equals `self.enhance(clip_i, solver=solver, atol=, rtol=)` bit for bit, NFE included (ragged STFT ->
        fd_ode_solve_adaptive_clips -> ragged iSTFT; `last_nfe_per_clip`, `last_rejected_per_clip`, `last_evals` as in `enhance`).  A
        batch-global controller would make a clip depend on its companions, so without the keyword they are refused."""
        fd_noise.exclusive(seeds=seeds, noise=noise, generator=generator)
        if solver in L.ADAPTIVE_SOLVERS and step_control != "clip":
            raise ValueError(f"enhance_batch: the adaptive solver {solver!r} runs in a batch with step_control='clip' only (per-clip step "
                             f"control); without it: fixed-step solvers only ({sorted(L.SOLVERS)})")
        if solver not in L.SOLVERS and solver not in L.ADAPTIVE_SOLVERS:
            raise ValueError(f"enhance_batch: unknown solver {solver!r}; supported: {sorted(L.SOLVERS) + sorted(L.ADAPTIVE_SOLVERS)}")
        per_clip = _check_step_control(step_control, solver, "enhance_batch")
        clips = list(clips)

        def launch(lib, h, io, B, Lrow, ws):
            z, sd = (io["noise"], None) if seeds is None else (None, io["seeds"])
            if per_clip:   # ragged STFT -> per-clip adaptive solve -> ragged iSTFT
                x_hat, _ = self._enhance_adaptive(lib, h, io["y"], z, sd, B, Lrow, N, sigma_fac, False, float(atol), float(rtol), L.ADAPTIVE_SOLVERS[solver],
                                                  True, lengths=[int(c.numel()) for c in clips])
                return x_hat.reshape(B, Lrow)
            if sd is not None:
                L.check(lib.fd_enhance_seeded(h, L.ptr(io["y"]), L.ptr(io["lens"]), L.ptr(sd), float(sigma_fac), int(N),
                                              L.SOLVERS[solver], L.ptr(io["out"]), B, Lrow, L.ptr(ws), ws.numel(), int(use_graph), L.stream()))
            else:
                L.check(lib.fd_enhance_ragged(h, L.ptr(io["y"]), L.ptr(io["lens"]), L.ptr(torch.view_as_real(z)), float(sigma_fac), int(N),
                                              L.SOLVERS[solver], L.ptr(io["out"]), B, Lrow, L.ptr(ws), ws.numel(), int(use_graph), L.stream()))
        return self._ragged_call(clips, 1, noise, generator, seeds, launch)

    def valid_loss(self, x, y, *, seed=None, noise=None, t=None, reduce: str = "mean", return_t: bool = False, comp_eps=None):
        """FlowModel._loss (model.py:421-468) on clean x / coded y of one length, without gradients: the `valid_loss` of validation_step.
        seed= (the library's noise and time), noise= [n_draws, B, 1, F, T_pad] (draw 0: Ys, draw 1: Xs when sigma_x != 0), t= [B];
        reduce='none' -> per-clip values (float64); return_t=True adds the times.  See flowdec_amd/loss.py."""
        return fd_loss.valid_loss(self, "flow", x, y, seed=seed, noise=noise, t=t, reduce=reduce, return_t=return_t, comp_eps=comp_eps)

    def valid_loss_batch(self, xs, ys, *, seeds=None, noise=None, t=None, reduce: str = "mean", return_t: bool = False, max_batch: int = 8):
        """`valid_loss` for lists of pairs of any lengths, bucketed by padded frame count; every pair bit-identical to its one-pair call."""
        return fd_loss.valid_loss_batch(self, "flow", xs, ys, seeds=seeds, noise=noise, t=t, reduce=reduce, return_t=return_t, max_batch=max_batch)

    def _chunks_call(self, N: int = 50, solver: str = "euler", sigma_fac: float = 1.0, who: str = "enhance_long", **unknown):
        """The long-form hook (see _WaveModel._chunks_call): fd_enhance_chunks with a fixed-step solver."""
        if unknown:
            raise ValueError(f"{who}: a flow model takes N, solver and sigma_fac (got {sorted(unknown)})")
        if solver not in L.SOLVERS:
            raise ValueError(f"{who}: fixed-step solvers only ({sorted(L.SOLVERS)}), got {solver!r}")
        N, sigma_fac, solver_id = int(N), float(sigma_fac), L.SOLVERS[solver]

        def call(lib, h, y, lens, seeds, frame0, normfac, out, B, Lrow, ws, use_graph):
            L.check(lib.fd_enhance_chunks(h, y, lens, seeds, frame0, normfac, sigma_fac, N, solver_id, out, B, Lrow, L.ptr(ws), ws.numel(),
                                          int(use_graph), L.stream()))
        return call

    @torch.no_grad()
    @_serialized
    @_normfac_option
    def enhance_long(self, y, N: int = 50, solver: str = "euler", sigma_fac: float = 1.0, seed=None, row_frames: int = 3712,
                     halo_frames: int = 256, xfade: Optional[int] = None, rows_per_call: int = 8, use_graph: bool = True):
        """`enhance` for a recording of ANY length in fixed device memory (no counterpart in the reference, whose driver skips files over
        30 s): the recording is cut into overlapping rows of `row_frames` frames (flowdec_amd.longform.plan_rows), the rows run through
        fd_enhance_chunks in groups of at most `rows_per_call` -- one workspace of (rows_per_call, row_frames) and one hipGraph whatever
        the length -- and fd_stitch_chunks cross-fades `xfade` samples (default 2 hops) around every boundary.

        y: [L], [1, L] or [C, 1, L]; several channels are independent recordings.  The recording is normalised ONCE, by its own maximum
        (fd_normfac; normalize_mode='none': not at all).  The noise is the library's own, addressed by the ABSOLUTE frame of the
        recording: `seed` as in `enhance(seed=)` (an int -> channel c uses clip_seed(seed, c); C ints; an int64 / uint64 tensor [C]),
        None draws one from torch's default generator.  Rows that overlap start from bit-identical noise in their overlap, so a seam is
        a cross-fade of two nearly equal signals.  A recording of one row equals `enhance(y, seed=seed)` bit for bit; the result does
        not depend on `rows_per_call`.  Fixed-step solvers only.  Returns a tensor with the shape and on the device of `y`.

        The two halves are callable on their own (`enhance_long_rows` -> `enhance_long_stitch`): a row's output depends on (recording,
        seed, absolute frame) only, so any split of the (channel, row) jobs over calls -- or over processes,
        `flowdec_amd.dist.sharded_enhance_long` -- stitches to the same bits.

        Keyword `normfac` (normalize_mode='noisy' only; added by @_normfac_option) replaces the recording's maximum: a float, or a tensor of one factor per channel; or
        "causal": row j is scaled by fd_normfac(y[0 : start_j + len_j)), the peak of everything up to the row's END -- the one
        normalisation a stream can reproduce (flowdec_amd.stream), as it depends on the samples up to there and on nothing else.
        Overlapping rows then differ slightly in scale; the cross-fade absorbs the difference.  None: the recording's maximum.

        The machinery is the base class's (`_WaveModel._enhance_long`), shared with the ScoreDec and regression models."""
        return self._enhance_long(y, self._chunks_call(N, solver, sigma_fac), seed, row_frames, halo_frames, xfade, rows_per_call, use_graph,
                                  normfac=self._long_normfac)

    @torch.no_grad()
    @_serialized
    @_normfac_option
    def enhance_long_rows(self, y, jobs: Optional[Tuple[int, int]] = None, N: int = 50, solver: str = "euler", sigma_fac: float = 1.0,
                          seed=None, row_frames: int = 3712, halo_frames: int = 256, xfade: Optional[int] = None, rows_per_call: int = 8,
                          use_graph: bool = True):
        """The first half of `enhance_long`: the outputs of the jobs [lo, hi) = `jobs` (default: all) of the recording's job pool -- job
        c * R + j is row j of channel c, R rows per channel -- as a float32 device tensor [hi - lo, row samples] (row k holds the samples
        from its row's start on; what lies beyond the row's length is unspecified).  `seed` must be given: the rows of one recording
        share it.  The normalisation is the whole recording's whichever jobs run (a maximum: the same bits in every call); `normfac` as
        in `enhance_long` (with "causal", overlapping rows differ slightly in scale; the cross-fade of the stitch absorbs it)."""
        return self._enhance_long_rows(y, self._chunks_call(N, solver, sigma_fac), jobs, seed, row_frames, halo_frames, xfade, rows_per_call,
                                       use_graph, normfac=self._long_normfac)

    def enhance_long_stitch(self, y, row_out, row_frames: int = 3712, halo_frames: int = 256, xfade: Optional[int] = None):
        """The second half of `enhance_long`: the recording from the outputs of ALL its jobs (`enhance_long_rows`, in job order).  Only the
        shape, the device and the length of `y` are used."""
        return self._enhance_long_stitch(y, row_out, row_frames, halo_frames, xfade)

    def enhance_long_jobs(self, y, row_frames: int = 3712, halo_frames: int = 256, xfade: Optional[int] = None) -> int:
        """The number of (channel, row) jobs `enhance_long` cuts y into."""
        return self._enhance_long_jobs(y, row_frames, halo_frames, xfade)

    def _enhance_adaptive(self, lib, h, y_rows, noise, seeds, B, Lw, N, sigma_fac, return_traj, atol, rtol, method, per_clip, lengths=None):
        """solver='dopri5' / 'tsit5' on the staged rows y_rows [B, Lw]: adaptive 5(4) pair over t_span = linspace(0, 1, N+1) (torchdyn
        semantics restated, unpinned); host-driven (one read-back per attempted step), so no hipGraph.  The realised NFE is left in
        `self.last_nfe`.  per_clip: every clip under its own controller (fd_ode_solve_adaptive_clips); then `seeds` (device int64 [B])
        may replace `noise` ([1, B, 1, F, Tp]), and `lengths` makes the batch ragged (clip b = the first lengths[b] samples of its row).
        -> (x_hat [B, 1, Lw], normfac [B]), or with return_traj (the trajectory, its waveforms)."""
        cfg, dev = self.feature_extractor._cfg(), y_rows.device
        F, T, Tp = self._frames(Lw)
        Y, normfac, _ = ops.stft_compress(y_rows, normalize=self.normalize_mode == "noisy", lengths=lengths, **cfg)
        traj = torch.empty(N + 1, B, 1, F, Tp, dtype=torch.complex64, device=dev) if return_traj else None
        X = torch.empty_like(Y)
        traj_ptr = L.ptr(torch.view_as_real(traj)) if return_traj else None
        noise_ptr = None if seeds is not None else L.ptr(torch.view_as_real(noise))
        if per_clip:
            need = lib.fd_ode_adaptive_clips_workspace_bytes(h, B, Tp)
            if need == 0:
                raise RuntimeError(f"flowdec_hip: step_control='clip' takes at most 256 clips of a valid shape per call (got B={B}, T_pad={Tp})")
            ws = self.backbone.workspace(("ode", B, Tp), need, dev)
            nfe, rej, evals = (C.c_int * B)(), (C.c_int * B)(), C.c_int(0)
            L.check(lib.fd_ode_solve_adaptive_clips(h, L.ptr(torch.view_as_real(Y)), noise_ptr, L.ptr(seeds), float(sigma_fac), int(N), int(method), atol, rtol,
                                                    L.ptr(torch.view_as_real(X)), traj_ptr, nfe, rej, C.byref(evals), B, Tp, L.ptr(ws), ws.numel(), L.stream()))
            self.last_nfe_per_clip = torch.tensor(list(nfe), dtype=torch.int64)
            self.last_rejected_per_clip = torch.tensor(list(rej), dtype=torch.int64)
            self.last_evals = int(evals.value)
            self.last_nfe = int(self.last_nfe_per_clip.max())
        else:
            need = lib.fd_ode_adaptive_workspace_bytes(h, B, Tp)
            ws = self.backbone.workspace(("ode", B, Tp), need, dev)
            nfe = C.c_int(0)
            L.check(lib.fd_ode_solve_adaptive_method(h, L.ptr(torch.view_as_real(Y)), noise_ptr, float(sigma_fac), int(N), int(method),
                                                     atol, rtol, L.ptr(torch.view_as_real(X)), traj_ptr, C.byref(nfe), B, Tp, L.ptr(ws), ws.numel(), L.stream()))
            self.last_nfe = int(nfe.value)
        if return_traj:
            return traj, _traj_waveforms(traj, T, Lw, normfac, cfg, lengths)
        return ops.decompress_istft(X, T, Lw, normfac, lengths=lengths, **cfg).reshape(B, 1, Lw), normfac

    def _enhance_traj(self, lib, h, y_rows, noise, seeds, B, Lw, N, solver, sigma_fac):
        """A fixed-step solve that keeps every solver state: front end, solver and back end as separate native calls; `seeds` (device int64
        [B]) selects the seeded solver, which reads no noise.  -> (the trajectory, its waveforms)."""
        cfg, dev = self.feature_extractor._cfg(), y_rows.device
        F, T, Tp = self._frames(Lw)
        Y, normfac, _ = ops.stft_compress(y_rows, normalize=self.normalize_mode == "noisy", **cfg)
        traj = torch.empty(N + 1, B, 1, F, Tp, dtype=torch.complex64, device=dev)
        X = torch.empty_like(Y)
        ws = self.backbone.workspace(("ode", B, Tp), lib.fd_model_workspace_bytes(h, B, Tp), dev)
        solve, src = (lib.fd_ode_solve, torch.view_as_real(noise)) if seeds is None else (lib.fd_ode_solve_seeded, seeds)
        L.check(solve(h, L.ptr(torch.view_as_real(Y)), L.ptr(src), float(sigma_fac), int(N), L.SOLVERS[solver], L.ptr(torch.view_as_real(X)),
                      L.ptr(torch.view_as_real(traj)), B, Tp, L.ptr(ws), ws.numel(), 0, L.stream()))
        return traj, _traj_waveforms(traj, T, Lw, normfac, cfg)


# ------------------------------------------------------------------------------------------------
# ScoreDec / regression baselines on the same backbone
# ------------------------------------------------------------------------------------------------
class OUVESDE:
    """flowdec.sdes.OUVESDE (sdes.py:132-206): parameters + the closed forms the sampler needs (float32 like the reference)."""

    def __init__(self, theta, sigma_min, sigma_max, N=1000, **ignored_kwargs):
        self.theta, self.sigma_min, self.sigma_max, self.N = float(theta), float(sigma_min), float(sigma_max), int(N)
        self.logsig = float(np.log(self.sigma_max / self.sigma_min))

    def copy(self):
        return OUVESDE(self.theta, self.sigma_min, self.sigma_max, N=self.N)

    @property
    def T(self):
        return 1

    def _std(self, t: torch.Tensor) -> torch.Tensor:                       # sdes.py:181-192
        th, ls = self.theta, self.logsig
        return torch.sqrt(self.sigma_min ** 2 * torch.exp(-2 * th * t) * (torch.exp(2 * (th + ls) * t) - 1) * ls / (th + ls))

    def _mean(self, x0, t, y):                                            # sdes.py:176-179
        e = torch.exp(-self.theta * t)[:, None, None, None]
        return e * x0 + (1 - e) * y

    def marginal_prob(self, x0, t, y):
        return self._mean(x0, t, y), self._std(t)


class ScoreModel(_WaveModel):
    """Drop-in for flowdec.model.ScoreModel on the inference path (model.py:581-690): `forward` = score estimate,
    `enhance` = predictor-corrector sampling (sampler_type='pc').  Extensions: noise= / generator= / seed= / use_graph=; with `seed=`
    (see FlowModel) the sampler's Gaussian planes are generated inside its update kernels and no noise tensor is allocated."""

    def __init__(self, sde: OUVESDE, t_eps: float, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.sde, self.t_eps = sde, t_eps

    def sde_std(self, t_batch):
        return self.sde._std(t_batch)

    def forward(self, xt, y, t_batch):
        """-backbone(xt, y, t) / std(t)  (model.py:613-628)."""
        if t_batch.ndim == 0:
            t_batch = t_batch.unsqueeze(0)
        self._sync_native()
        std = self.sde_std(t_batch.float())
        return -self.backbone(xt, y, t_batch) / std.reshape(-1, 1, 1, 1)

    def valid_loss(self, x, y, *, seed=None, noise=None, t=None, reduce: str = "mean", return_t: bool = False, comp_eps=None):
        """ScoreModel._loss (model.py:590-611) without gradients; the time is drawn over [t_eps, 1).  See FlowModel.valid_loss."""
        return fd_loss.valid_loss(self, "score", x, y, seed=seed, noise=noise, t=t, reduce=reduce, return_t=return_t, comp_eps=comp_eps)

    def valid_loss_batch(self, xs, ys, *, seeds=None, noise=None, t=None, reduce: str = "mean", return_t: bool = False, max_batch: int = 8):
        return fd_loss.valid_loss_batch(self, "score", xs, ys, seeds=seeds, noise=noise, t=t, reduce=reduce, return_t=return_t, max_batch=max_batch)

    def _pc_config(self, predictor, corrector, N, corrector_steps, snr, denoise, eps=None):
        """-> (fd_score_config of the predictor-corrector sampler, the number of Gaussian planes it consumes)."""
        if predictor not in L.PREDICTORS:
            raise ValueError(f"unknown predictor {predictor!r}; supported: {sorted(L.PREDICTORS)}")
        if corrector not in L.CORRECTORS:
            raise ValueError(f"unknown corrector {corrector!r}; supported: {sorted(L.CORRECTORS)}")
        N = self.sde.N if N is None else int(N)
        cfg = L.FdScoreConfig(self.sde.theta, self.sde.sigma_min, self.sde.sigma_max, float(self.t_eps if eps is None else eps), float(snr), N,
                              L.PREDICTORS[predictor], L.CORRECTORS[corrector], int(corrector_steps), int(bool(denoise)))
        return cfg, self.num_draws(N, predictor, corrector, corrector_steps)

    def num_draws(self, N=None, predictor="reverse_diffusion", corrector="ald", corrector_steps=1) -> int:
        N = self.sde.N if N is None else N
        return 1 + N * ((corrector_steps if corrector == "ald" else 0) + (1 if predictor != "none" else 0))

    @torch.no_grad()
    def enhance(self, y, sampler_type="pc", predictor="reverse_diffusion", corrector="ald", N=30, corrector_steps=1, snr=0.5,
                return_preprocess_info=False, denoise=True, noise=None, generator=None, use_graph: bool = True, seed=None, **kwargs):
        fd_noise.exclusive(seed=seed, noise=noise, generator=generator)
        if sampler_type == "ode":
            return self._enhance_ode(y, N=N, denoise=denoise, noise=noise, generator=generator, seed=seed, return_preprocess_info=return_preprocess_info, **kwargs)
        if sampler_type != "pc":
            raise ValueError(f"{sampler_type} is not a valid sampler type!")
        cfg, n_draws = self._pc_config(predictor, corrector, N, corrector_steps, snr, denoise, kwargs.get("eps"))

        def launch(lib, h, io, B, Lw, ws):
            assert lib.fd_score_num_draws(C.byref(cfg)) == n_draws
            if seed is not None:
                L.check(lib.fd_score_enhance_seeded(h, L.ptr(io["y"]), L.ptr(io["seeds"]), C.byref(cfg), L.ptr(io["out"]), B, Lw,
                                                    L.ptr(ws), ws.numel(), int(use_graph), L.stream()))
            else:
                L.check(lib.fd_score_enhance(h, L.ptr(io["y"]), L.ptr(torch.view_as_real(io["noise"])), C.byref(cfg), L.ptr(io["out"]), B, Lw,
                                             L.ptr(ws), ws.numel(), int(use_graph), L.stream()))
        return self._wave_call(y, n_draws, noise, generator, launch, return_preprocess_info, seed=seed)

    @torch.no_grad()
    def enhance_batch(self, clips, predictor="reverse_diffusion", corrector="ald", N=30, corrector_steps=1, snr=0.5, denoise=True,
                      noise=None, generator=None, seeds=None, use_graph: bool = True, **kwargs):
        """`[self.enhance(c, ...) for c in clips]` as ONE native call (fd_score_enhance_ragged) for clips of DIFFERENT lengths whose
        spectrograms pad to the same T_pad (the bucket rule and the errors of FlowModel.enhance_batch).  Every clip's result is
        BIT-IDENTICAL to `self.enhance(clip)` with the same noise.  `noise` = one [n_draws, 1, 1, F, T_pad] complex tensor per clip
        (n_draws = self.num_draws(...)), or `generator` = one torch.Generator (drawn clip by clip) or a list of one per clip -- clip b's
        planes are then one draw of that shape, exactly what `enhance(clip_b, generator=g_b)` draws --, or `seeds` = one 64-bit seed
        per clip: clip i equals `self.enhance(clip_i, seed=[seeds[i]])`.  Only the predictor-corrector sampler runs here; the ODE sampler
        has its own batch entry point, `enhance_ode_batch` (one step controller per clip)."""
        fd_noise.exclusive(seeds=seeds, noise=noise, generator=generator)
        sampler_type = kwargs.get("sampler_type", "pc")
        if sampler_type != "pc":
            raise ValueError(f"enhance_batch: sampler_type='pc' only (got {sampler_type!r}); the 'ode' sampler is host-driven: call enhance() per clip")
        cfg, n_draws = self._pc_config(predictor, corrector, N, corrector_steps, snr, denoise, kwargs.get("eps"))

        def launch(lib, h, io, B, Lrow, ws):
            assert lib.fd_score_num_draws(C.byref(cfg)) == n_draws
            L.check(lib.fd_score_enhance_ragged(h, L.ptr(io["y"]), L.ptr(io["lens"]), None if seeds is not None else L.ptr(torch.view_as_real(io["noise"])),
                                                L.ptr(io["seeds"]) if seeds is not None else None, C.byref(cfg), L.ptr(io["out"]), B, Lrow,
                                                L.ptr(ws), ws.numel(), int(use_graph), L.stream()))
        return self._ragged_call(clips, n_draws, noise, generator, seeds, launch)

    def _chunks_call(self, predictor="reverse_diffusion", corrector="ald", N=30, corrector_steps=1, snr=0.5, denoise=True, sampler_type="pc",
                     eps=None, who: str = "enhance_long", **unknown):
        """The long-form hook (see _WaveModel._chunks_call): fd_score_enhance_chunks -- the predictor-corrector sampler with every one of its
        draws taken at the absolute frame.  The ODE sampler is refused: its per-clip step control would give two overlapping rows
        different step sequences (no common noise-free trajectory to cross-fade), and it is synchronous."""
        if unknown:
            raise ValueError(f"{who}: a score model takes the sampler arguments predictor, corrector, N, corrector_steps, snr and denoise "
                             f"(got {sorted(unknown)}; `solver` and `sigma_fac` belong to the flow model)")
        if sampler_type != "pc":
            raise ValueError(f"{who}: sampler_type='pc' only (got {sampler_type!r}); the 'ode' sampler has no long-form: every row would take "
                             f"its own adaptive steps, and the driver is synchronous")
        cfg, _ = self._pc_config(predictor, corrector, N, corrector_steps, snr, denoise, eps)

        def call(lib, h, y, lens, seeds, frame0, normfac, out, B, Lrow, ws, use_graph):
            L.check(lib.fd_score_enhance_chunks(h, y, lens, seeds, frame0, normfac, C.byref(cfg), out, B, Lrow, L.ptr(ws), ws.numel(),
                                                int(use_graph), L.stream()))
        return call

    def _ode_config(self, N, denoise, eps, rtol, atol, who):
        """-> (fd_score_config of the ODE sampler, rtol, atol); the tolerances are checked here, before the device is touched."""
        rtol, atol = float(rtol), float(atol)
        if not atol > 0.0 or not rtol >= 0.0:
            raise ValueError(f"{who}: need atol > 0 and rtol >= 0 (got atol={atol}, rtol={rtol})")
        N = self.sde.N if N is None else int(N)
        t_eps = float(self.t_eps if eps is None else eps)
        return L.FdScoreConfig(self.sde.theta, self.sde.sigma_min, self.sde.sigma_max, t_eps, 0.0, N, 0, 1, 0, int(bool(denoise))), rtol, atol

    def _ode_launch(self, sc, rtol, atol, per_clip, seeded, ragged, stats):
        """The `launch` closure of the device-driven ODE sampler: ONE fd_score_ode_enhance call on the staged rows (its own workspace: the
        adaptive driver's ten state planes do not fit the enhance calls').  Leaves nfe / rejected (lists) and evals in `stats`."""
        def launch(lib, h, io, B, Lrow, _):
            ctl = L.STEP_CONTROL["clip" if per_clip else "batch"]
            need = lib.fd_score_ode_enhance_workspace_bytes(h, B, Lrow, ctl)
            if need == 0:
                raise RuntimeError(f"flowdec_hip: the ODE sampler takes at most 256 clips of a valid shape per call with per-clip step control "
                                   f"(got B={B}, L={Lrow})")
            ws = self.backbone.workspace(("score_ode", B, Lrow), need, io["y"].device)
            n = B if per_clip else 1
            nfe, rej, evals = (C.c_int * n)(), (C.c_int * n)(), C.c_int(0)
            L.check(lib.fd_score_ode_enhance(h, L.ptr(io["y"]), L.ptr(io["lens"]) if ragged else None,
                                             None if seeded else L.ptr(torch.view_as_real(io["noise"])), L.ptr(io["seeds"]) if seeded else None,
                                             C.byref(sc), rtol, atol, ctl, L.ptr(io["out"]), nfe, rej, C.byref(evals), B, Lrow, L.ptr(ws), ws.numel(),
                                             L.stream()))
            stats.update(nfe=list(nfe), rejected=list(rej), evals=int(evals.value))
            self.last_nfe, self.last_evals = max(stats["nfe"]), stats["evals"]
            self.last_nfe_per_clip = torch.tensor(stats["nfe"], dtype=torch.int64) if per_clip else None
            self.last_rejected_per_clip = torch.tensor(stats["rejected"], dtype=torch.int64) if per_clip else None
            if ragged:
                return None
            off = lib.fd_enhance_normfac_offset(h, B, Lrow)   # the layout's head (Y | X | normfac) is the enhance calls'
            return io["out"].reshape(B, 1, Lrow).clone(), ws[off:off + 4 * B].view(torch.float32).clone()
        return launch

    def _enhance_ode_device(self, y, N, denoise, noise, generator, seed, rtol, atol, method, eps, return_nfe, return_preprocess_info, extra):
        """sampler_type='ode', driver='device': the whole sampler as ONE native call (fd_score_ode_enhance) -- STFT, the prior sample, the
        Dormand-Prince 5(4) solve of the probability-flow ODE under scipy RK45's own step-size rule with ONE controller for the batch
        (what solve_ivp sees in the host driver: the reference's meaning of a batch), the denoising step, iSTFT.  The state stays on the
        device in float32 planes (scipy carries complex128 on the host); NFE is scipy's count.  A step below ten spacings of t raises
        ("step size too small") where scipy stops with a failure status and the reference goes on with the last state."""
        if method != "RK45":
            raise ValueError(f"enhance(sampler_type='ode', driver='device'): method='RK45' only (got {method!r}); other scipy methods run with driver='host'")
        if extra:
            raise ValueError(f"enhance(sampler_type='ode', driver='device'): unsupported solve_ivp option(s) {sorted(extra)}; they run with driver='host'")
        sc, rtol, atol = self._ode_config(N, denoise, eps, rtol, atol, "enhance(sampler_type='ode', driver='device')")
        stats = {}
        res = self._wave_call(y, 1, noise, generator, self._ode_launch(sc, rtol, atol, False, seed is not None, False, stats),
                              return_preprocess_info, seed=seed)
        if return_preprocess_info:
            return res
        return (res, stats["nfe"][0]) if return_nfe else res

    @torch.no_grad()
    def enhance_ode_batch(self, clips, N=30, rtol=1e-5, atol=1e-5, denoise=True, eps=None, noise=None, generator=None, seeds=None,
                          return_nfe: bool = False):
        """The ODE sampler on clips of DIFFERENT lengths whose spectrograms pad to one T_pad (the bucket rule of `enhance_batch`), as ONE
        native call with ONE step-size controller PER CLIP: clip b takes the steps of, and is BIT-IDENTICAL to,
        `self.enhance(clip_b, sampler_type='ode', driver='device', ...)` with the same noise or seed, in any batch and in any order; a clip
        that has reached t_eps rides along (dt = 0) until the slowest one is done.  `noise` = one [1, 1, F, T_pad] complex tensor per clip,
        `generator` = one torch.Generator (drawn clip by clip) or one per clip, `seeds` = one 64-bit seed per clip (clip i equals
        `enhance(clip_i, ..., seed=[seeds[i]])`).  At most 256 clips per call.  -> list of waveforms; with return_nfe also the per-clip NFE
        (list of int).  `last_nfe_per_clip`, `last_rejected_per_clip`, `last_evals` as in FlowModel.enhance."""
        fd_noise.exclusive(seeds=seeds, noise=noise, generator=generator)
        sc, rtol, atol = self._ode_config(N, denoise, eps, rtol, atol, "enhance_ode_batch")
        stats = {}
        outs = self._ragged_call(clips, 1, noise, generator, seeds, self._ode_launch(sc, rtol, atol, True, seeds is not None, True, stats))
        return (outs, stats.get("nfe", [])) if return_nfe else outs

    @_serialized
    def _enhance_ode(self, y, N=None, denoise=True, noise=None, generator=None, seed=None, rtol=1e-5, atol=1e-5, method="RK45", eps=None,
                     return_nfe: bool = False, return_preprocess_info: bool = False, driver: str = "host", **ignored):
        """sampler_type='ode' (sampling/__init__.py:75-146): the probability-flow ODE integrated by scipy.integrate.solve_ivp
        on the host, exactly like the reference; every drift evaluation is one fd_score_eval (backbone + fused update) on
        the GPU, the STFT / iSTFT run in libflowdec_hip.so.  Host-driven and slow by construction (the state crosses PCIe
        twice per evaluation) -- it exists for API parity with ScoreModel.enhance.  driver='device' (`_enhance_ode_device`) runs the
        same sampler, method 'RK45', entirely on the GPU."""
        if driver == "device":
            return self._enhance_ode_device(y, N, denoise, noise, generator, seed, rtol, atol, method, eps, return_nfe, return_preprocess_info, ignored)
        if driver != "host":
            raise ValueError(f"enhance(sampler_type='ode'): driver must be 'host' or 'device' (got {driver!r})")
        from scipy import integrate
        dev = self._gpu()
        orig_device = y.device
        y3, squeeze_dims = _to_3d(y, "enhance expects")
        N = self.sde.N if N is None else int(N)
        t_eps = float(self.t_eps if eps is None else eps)
        lib = L.load()
        h = self._sync_native()
        cfg = self.feature_extractor._cfg()
        B, Lw = y3.shape[0], y3.shape[-1]
        sc = L.FdScoreConfig(self.sde.theta, self.sde.sigma_min, self.sde.sigma_max, t_eps, 0.0, N, 0, 1, 0, int(bool(denoise)))
        with torch.cuda.device(dev):
            Y, normfac, T = ops.stft_compress(y3.reshape(B, Lw).to(dev, torch.float32), normalize=self.normalize_mode == "noisy", **cfg)
            Tp = Y.shape[-1]
            if seed is not None:   # the prior draw (index 0) of the seeded noise; the ODE itself is noise-free
                noise = fd_noise.noise_fill(fd_noise.seeds_to_tensor(seed, B, dev), Y.shape[-2], Tp)[0]
            elif noise is None:
                noise = torch.randn(Y.shape, dtype=torch.complex64, device=dev, generator=generator)
            std1 = float(self.sde._std(torch.ones(1))[0])
            # prior sample x_T = Y + std(1) * z (sdes.py:197-202), formed on the host where scipy keeps the state anyway
            x0 = (Y.cpu().numpy() + noise.to("cpu", torch.complex64).reshape(Y.shape).numpy() * np.float32(std1)).astype(np.complex64)
            ws = self.backbone.workspace(("fwd", B, Tp), lib.fd_model_workspace_bytes(h, B, Tp), dev)
            xin, out = torch.empty_like(Y), torch.empty_like(Y)

            def evaluate(x_host, t, mode):
                xin.copy_(torch.from_numpy(np.ascontiguousarray(x_host.reshape(Y.shape).astype(np.complex64))))
                L.check(lib.fd_score_eval(h, L.ptr(torch.view_as_real(xin)), L.ptr(torch.view_as_real(Y)), float(np.float32(t)), C.byref(sc), mode,
                                          L.ptr(torch.view_as_real(out)), B, Tp, L.ptr(ws), ws.numel(), L.stream()))
                return out.cpu().numpy().reshape(-1)

            sol = integrate.solve_ivp(lambda t, xf: evaluate(xf, t, 0), (1.0, t_eps), x0.reshape(-1), rtol=rtol, atol=atol, method=method)
            x = sol.y[:, -1]
            if denoise:
                x = evaluate(x, t_eps, 2)
            X = torch.from_numpy(np.ascontiguousarray(x.reshape(Y.shape).astype(np.complex64))).to(dev)
            x_hat = ops.decompress_istft(X, T, Lw, normfac, **cfg).reshape(B, 1, Lw)
        for _ in range(squeeze_dims):
            x_hat = x_hat.squeeze(0)
        x_hat = x_hat.to(orig_device)
        if return_preprocess_info:
            return x_hat, _preprocess_info(Lw, normfac, T, squeeze_dims)
        return (x_hat, int(sol.nfev)) if return_nfe else x_hat


class RegressionModel(_WaveModel):
    """Drop-in for flowdec.model.RegressionModel.enhance (model.py:539-578): one backbone call with x_t = Y, t = 0."""

    _draws_noise = False

    def __init__(self, *args, loss_type: str = "l2", **kwargs):
        super().__init__(*args, **kwargs)
        self.loss_type = loss_type

    def _chunks_call(self, who: str = "enhance_long", **unknown):
        """The long-form hook (see _WaveModel._chunks_call): fd_regression_enhance_chunks.  No sampler, no seed: seeds and frame0 are not read."""
        if unknown:
            raise ValueError(f"{who}: a regression model makes one network evaluation per row and takes no sampler arguments (got {sorted(unknown)})")

        def call(lib, h, y, lens, seeds, frame0, normfac, out, B, Lrow, ws, use_graph):
            L.check(lib.fd_regression_enhance_chunks(h, y, lens, normfac, out, B, Lrow, L.ptr(ws), ws.numel(), int(use_graph), L.stream()))
        return call

    def forward(self, xt, y, t):
        if t.ndim == 0:
            t = t.unsqueeze(0)
        self._sync_native()
        return self.backbone(xt, y, t)

    def valid_loss(self, x, y, *, reduce: str = "mean", comp_eps=None):
        """RegressionModel._loss (model.py:552-559) without gradients: mean |backbone(Y, Y, 0) - X|^2.  No random draws."""
        return fd_loss.valid_loss(self, "regression", x, y, reduce=reduce, comp_eps=comp_eps)

    def valid_loss_batch(self, xs, ys, *, reduce: str = "mean", max_batch: int = 8):
        return fd_loss.valid_loss_batch(self, "regression", xs, ys, reduce=reduce, max_batch=max_batch)

    @torch.no_grad()
    def enhance(self, y, return_preprocess_info=False, use_graph: bool = True, **kwargs):
        def launch(lib, h, io, B, Lw, ws):
            L.check(lib.fd_regression_enhance(h, L.ptr(io["y"]), L.ptr(io["out"]), B, Lw, L.ptr(ws), ws.numel(), int(use_graph), L.stream()))
        return self._wave_call(y, 0, None, None, launch, return_preprocess_info)

    @torch.no_grad()
    def enhance_batch(self, clips, use_graph: bool = True):
        """`[self.enhance(c) for c in clips]` as ONE native call (fd_regression_enhance_ragged) for clips of different lengths in one T_pad
        bucket (the bucket rule and the errors of FlowModel.enhance_batch); every result is bit-identical to the one-clip call."""
        def launch(lib, h, io, B, Lrow, ws):
            L.check(lib.fd_regression_enhance_ragged(h, L.ptr(io["y"]), L.ptr(io["lens"]), L.ptr(io["out"]), B, Lrow, L.ptr(ws), ws.numel(),
                                                     int(use_graph), L.stream()))
        return self._ragged_call(clips, 0, None, None, None, launch)


# ------------------------------------------------------------------------------------------------
# presets (replace hydra.compose('flowdec_75m' | 'flowdec_25s'), config/flowdec_75m.yaml etc.)
# ------------------------------------------------------------------------------------------------
BACKBONE_FINAL_NO_ATTN = dict(image_size=768, nonlinearity="swish", nf=64, ch_mult=(4, 4, 4, 2), num_res_blocks=1,
                              attn_resolutions=(), bottleneck_attn=False, resamp_with_conv=True, conditional=True, fir=True,
                              fir_kernel=(1, 3, 3, 1), skip_rescale=True, resblock_type="biggan", progressive="output_skip",
                              progressive_input="input_skip", progressive_combine="sum", init_scale=0.0, embedding_type="fourier",
                              fourier_scale=16, dropout=0.0, num_channels=4,
                              output_layer_kwargs=dict(kernel_size=1, bias=False, padding="same", padding_mode="zeros"))

# config/model/backbone/ncsnpp_default_ycond.yaml: the SGMSE+ backbone (flow_model_sgmse / score_model_sgmse)
BACKBONE_SGMSE = dict(image_size=768, nonlinearity="swish", nf=128, ch_mult=(1, 1, 2, 2, 2, 2, 2), num_res_blocks=2,
                      attn_resolutions=(), bottleneck_attn=True, resamp_with_conv=True, conditional=True, fir=True,
                      fir_kernel=(1, 3, 3, 1), skip_rescale=True, resblock_type="biggan", progressive="output_skip",
                      progressive_input="input_skip", progressive_combine="sum", init_scale=0.0, embedding_type="fourier",
                      fourier_scale=16, dropout=0.0, num_channels=4,
                      output_layer_kwargs=dict(kernel_size=3, bias=False, padding="same", padding_mode="zeros"))
# feature_extractor/compressed_complex_stft_sgmse1534.yaml
STFT_SGMSE = dict(alpha=0.5, beta=0.15)

PRESETS = {
    "flowdec_75m": dict(sigma_file="flowdec_autoparams_75m.npy"),
    "flowdec_25s": dict(sigma_file="flowdec_autoparams_25s.npy"),
    "flowdec_75m_globsigy": dict(sigma_file=None),
    "flowdec_25s_globsigy": dict(sigma_file=None),
    # baselines (config/baseline_scoredec_75s.yaml -> model/score_model_final.yaml + sde/ouve_final.yaml; baseline_regression_75s.yaml)
    "baseline_scoredec_75s": dict(kind="score", sde=dict(theta=1.5, sigma_min=0.05, sigma_max=0.82, N=30), t_eps=3e-2),
    "baseline_regression_75s": dict(kind="regression"),
    # config/model/flow_model_sgmse.yaml, score_model_sgmse.yaml (+ sde/ouve_sgmse.yaml): the SGMSE-style backbone and features
    "flow_model_sgmse": dict(sigma_file=None, sigma_y=0.5, backbone=BACKBONE_SGMSE, stft=STFT_SGMSE),
    "score_model_sgmse": dict(kind="score", sde=dict(theta=1.5, sigma_min=0.05, sigma_max=0.5, N=30), t_eps=3e-2, backbone=BACKBONE_SGMSE,
                              stft=STFT_SGMSE),
}


def from_preset(name: str = "flowdec_75m", precision: str = "bf16", **backbone_overrides):
    """Instantiate the model a reference user gets from `instantiate(compose(config_name=name)['model'])`."""
    if name not in PRESETS:
        raise KeyError(f"unknown preset {name!r}; available: {sorted(PRESETS)}")
    bb = dict(PRESETS[name].get("backbone", BACKBONE_FINAL_NO_ATTN)); bb.update(backbone_overrides)
    backbone = NCSNpp(precision=precision, **bb)
    stft = dict(alpha=0.3, beta=0.33); stft.update(PRESETS[name].get("stft", {}))
    fe = AmplitudeCompressedComplexSTFT(window_fn="hann", n_fft=1534, n_hops=4, sampling_rate=48000, **stft)
    kind = PRESETS[name].get("kind", "flow")
    if kind == "score":
        return ScoreModel(sde=OUVESDE(**PRESETS[name]["sde"]), t_eps=PRESETS[name]["t_eps"], backbone=backbone, feature_extractor=fe,
                          sampling_rate=48000).eval()
    if kind == "regression":
        return RegressionModel(backbone=backbone, feature_extractor=fe, sampling_rate=48000).eval()
    sf = PRESETS[name]["sigma_file"]
    sigma_y = sigma_y_from_file(sf, factor=1, kernel_bandwidth=3) if sf else PRESETS[name].get("sigma_y", 0.66)
    return FlowModel(backbone=backbone, feature_extractor=fe, sampling_rate=48000, sigma_x=0.0, sigma_y=sigma_y).eval()
