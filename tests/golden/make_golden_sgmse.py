#!/usr/bin/env python
"""Golden vectors for the SGMSE-style backbone (config/model/backbone/ncsnpp_default_ycond.yaml: nf 128, ch_mult
(1,1,2,2,2,2,2), two ResBlocks per level, one AttnBlockpp at the bottleneck, 3x3 output layer), produced by running the
REFERENCE modules (NCSNpp, layerspp.AttnBlockpp, FlowModel, ScoreModel) on CPU with the import recipe of make_golden.py.

Neither weights nor inputs are stored: `random_params(seed, shapes)` derives the weights from a seed and the parameter layout, and
`attn_input` / `forward_inputs` / `enhance_inputs` / `score_input` derive the inputs from seeds (the tests import this file with
importlib; a checksum of every input is stored to pin the re-derivation).  Large outputs are stored as the regular sample
`sample(a) = a.ravel()[::sample_step(a.size)]` (about 16k elements; its relative L2 error estimates the full one to ~1 %), small
ones whole.  The bf16 error prediction (g30) is derived, not fitted: the reference run again with bf16 rounding where the HIP bf16 mode
rounds -- every convolution's input (activations are stored in bf16) and, except for the input convolution and the
pyramid-combine 1x1 (f32 weights there), its weights; every convolution's, ResBlock's, Combine's and attention block's output
(stored in bf16), except the pyramid heads' (C -> 4), whose result is stored once with the upsampled pyramid added; the FIR-resampled
input and output pyramids (stored in bf16).  The attention block itself and the output layer compute in f32 on the stored tensors.

    python tests/golden/make_golden_sgmse.py   # writes tests/golden/{state_dict_manifest_sgmse.json, g26..g30}
"""
import contextlib
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

BB_SGMSE = dict(image_size=768, nonlinearity="swish", ch_mult=(1, 1, 2, 2, 2, 2, 2), num_res_blocks=2, attn_resolutions=[],
                bottleneck_attn=True, resamp_with_conv=True, conditional=True, fir=True, fir_kernel=[1, 3, 3, 1], skip_rescale=True,
                resblock_type="biggan", progressive="output_skip", progressive_input="input_skip", progressive_combine="sum",
                init_scale=0.0, embedding_type="fourier", fourier_scale=16, dropout=0.0, num_channels=4,
                output_layer_kwargs=dict(kernel_size=3, bias=False, padding="same", padding_mode="zeros"))
FE_SGMSE = dict(window_fn="hann", n_fft=1534, n_hops=4, sampling_rate=48000, alpha=0.5, beta=0.15)
ATTN_SHAPES = ((2, 12, 1), (1, 12, 4), (1, 12, 59))   # (B, H, W) at C = 256
ATTN_SEED, ATTN_BIG_LOGITS = 26, 6.0                  # big: NIN_0.W and NIN_1.W x 6 -> logits x 36
NOISE_SEED = 2929
SCORE_OUT_SCALE = 0.02


def random_params(seed, shapes, std=0.05):
    """Seeded weights for a parameter layout {name: shape} (iteration order matters): the time embedding's Fourier W ~ 16 N(0, 1)
    (fourier_scale), GroupNorm weights ~ 1 + N(0, .1), biases ~ N(0, std), NIN W ~ N(0, 1 / in), conv / linear weights ~ N(0, 1 / fan_in)."""
    rng = np.random.default_rng(seed)
    sd = {}
    for k, shp in shapes.items():
        shp = tuple(shp)
        if k.endswith("all_modules.0.W"):
            sd[k] = (rng.standard_normal(shp) * 16.0).astype(np.float32)
        elif "GroupNorm" in k and k.endswith("weight") or (len(shp) == 1 and k.endswith("weight")):
            sd[k] = (1.0 + 0.1 * rng.standard_normal(shp)).astype(np.float32)
        elif k.endswith("bias") or k.endswith(".b"):
            sd[k] = (std * rng.standard_normal(shp)).astype(np.float32)
        elif k.endswith(".W"):
            sd[k] = (rng.standard_normal(shp) / np.sqrt(shp[0])).astype(np.float32)
        else:
            sd[k] = (rng.standard_normal(shp) / np.sqrt(int(np.prod(shp[1:])))).astype(np.float32)
    return sd


def attn_params(C, big=False):
    shapes = {"GroupNorm_0.weight": (C,), "GroupNorm_0.bias": (C,)}
    for i in range(4):
        shapes[f"NIN_{i}.W"] = (C, C); shapes[f"NIN_{i}.b"] = (C,)
    sd = random_params(ATTN_SEED + (1 if big else 0), shapes)
    if big:
        for k in ("NIN_0.W", "NIN_1.W"):
            sd[k] = (sd[k] * np.float32(ATTN_BIG_LOGITS)).astype(np.float32)
    return sd


SAMPLE = 16384


def sample_step(n):
    return max(1, n // SAMPLE)


def sample(a):
    a = np.asarray(a).ravel()
    return np.ascontiguousarray(a[::sample_step(a.size)])


def crandn(rng, shape):
    """complex standard normal like torch.randn_like(complex): var 1/2 per part (as make_golden.crandn)."""
    return ((rng.standard_normal(shape) + 1j * rng.standard_normal(shape)) / np.sqrt(2.0)).astype(np.complex64)


def attn_input(B, H, W, big=False, C=256):
    """NCHW input of one G26 case."""
    rng = np.random.default_rng(2600 + 1000 * int(big) + 100 * B + W)
    return (1.3 * rng.standard_normal((B, C, H, W)) + 0.2).astype(np.float32)


def forward_inputs(nf):
    """x, y [2, 1, 768, 64] complex64 of G27 (nf 8) / G28 (nf 128)."""
    rng = np.random.default_rng(2700 + nf)
    return crandn(rng, (2, 1, 768, 64)), crandn(rng, (2, 1, 768, 64))


def enhance_inputs():
    """y [1, 1, 48000] and the initial noise [1, 1, 768, 128] of G29."""
    rng = np.random.default_rng(2900)
    y = (0.1 * rng.standard_normal((1, 1, 48000))).astype(np.float32)
    return y, crandn(rng, (1, 1, 768, 128))


def score_input():
    """y [2, 1, 12000] of the score-sampler case of G29."""
    y = (0.1 * np.random.default_rng(2930).standard_normal((2, 1, 12000))).astype(np.float32)
    y[1] *= 2.5
    return y


def checksum(a):
    a = np.asarray(a).astype(np.complex128 if np.iscomplexobj(a) else np.float64)
    return np.array([a.sum().real, a.sum().imag, (np.abs(a) ** 2).sum()])


def save_npz(path, **arrays):
    """np.savez_compressed with fixed zip timestamps, so that a re-run rewrites identical bytes."""
    import io
    import zipfile
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_DEFLATED) as z:
        for k, v in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(v), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(info, buf.getvalue())


def bf16(t):
    return t.to(torch.bfloat16).to(torch.float32)


@contextlib.contextmanager
def bf16_rounding(net):
    """The operand / storage rounding model of the HIP bf16 mode on a reference NCSNpp (see the module docstring)."""
    import torch.nn as nn
    from flowdec.backbones.ncsnpp_utils import layerspp
    hooks, saved = [], {}
    mods = list(net.all_modules)
    f32_weights = {id(mods[3])} | {id(m.Conv_0) for m in mods if isinstance(m, layerspp.Combine)}
    for m in net.all_modules.modules():
        if isinstance(m, nn.Conv2d):
            hooks.append(m.register_forward_pre_hook(lambda mod, inp: (bf16(inp[0]),) + tuple(inp[1:])))
            if m.out_channels != 4:   # a pyramid head: conv + upsampled pyramid are stored as one sum (read rounded by its consumers)
                hooks.append(m.register_forward_hook(lambda mod, inp, out: bf16(out)))
            if id(m) not in f32_weights:
                saved[m] = m.weight.data.clone()
                m.weight.data = bf16(m.weight.data)
        elif isinstance(m, (layerspp.ResnetBlockBigGANpp, layerspp.Combine, layerspp.AttnBlockpp)):
            hooks.append(m.register_forward_hook(lambda mod, inp, out: bf16(out)))
    # the FIR-resampled pyramids read and write stored tensors
    for m in (net.pyramid_upsample, net.pyramid_downsample):
        hooks.append(m.register_forward_pre_hook(lambda mod, inp: (bf16(inp[0]),) + tuple(inp[1:])))
        hooks.append(m.register_forward_hook(lambda mod, inp, out: bf16(out)))
    # the output layer reads the stored pyramid
    hooks.append(net.output_layer.register_forward_pre_hook(lambda mod, inp: (bf16(inp[0]),)))
    try:
        yield
    finally:
        for h in hooks:
            h.remove()
        for m, w in saved.items():
            m.weight.data = w


def rel(a, b):
    return float(np.linalg.norm((a - b).ravel()) / np.linalg.norm(b.ravel()))


def main():
    import make_golden as MG
    from oracle import flowdec_oracle as O
    torch.manual_seed(0)
    torch.set_grad_enabled(False)
    MG._install_stubs()
    from flowdec.backbones.ncsnpp import NCSNpp
    from flowdec.backbones.ncsnpp_utils import layerspp
    from flowdec.data.feature_extractors import AmplitudeCompressedComplexSTFT
    from flowdec.model import FlowModel, ScoreModel
    from flowdec.sdes import OUVESDE
    fe = AmplitudeCompressedComplexSTFT(**FE_SGMSE)
    pred = {}

    # ---- manifest: the reference FlowModel's state_dict at nf 128 -----------------------------------------------
    fm = FlowModel(flow_matcher=None, sigma_x=0.0, sigma_y=0.5, backbone=NCSNpp(nf=128, **BB_SGMSE), feature_extractor=fe,
                   sampling_rate=48000, lr=1e-4, full_config={}).eval()
    manifest = {k: list(v.shape) for k, v in fm.state_dict().items()}
    with open(os.path.join(HERE, "state_dict_manifest_sgmse.json"), "w") as f:
        json.dump(manifest, f, indent=0)
    bb_shapes = {k: v for k, v in manifest.items() if k.startswith("backbone.")}

    # ---- G26: AttnBlockpp, C = 256 -----------------------------------------------------------------------------
    g26 = {}
    for big in (False, True):
        blk = layerspp.AttnBlockpp(channels=256, skip_rescale=True, init_scale=0.0).eval()
        blk.load_state_dict(MG.to_t(attn_params(256, big)))
        for (B, H, W) in ATTN_SHAPES if not big else ATTN_SHAPES[2:]:
            nm = f"{'big_' if big else ''}{B}x{H}x{W}"
            x = attn_input(B, H, W, big)
            o = blk(torch.from_numpy(x)).numpy()
            g26[nm + "_x_sum"] = checksum(x)
            g26[nm + "_out" if o.size <= SAMPLE else nm + "_out_s"] = o if o.size <= SAMPLE else sample(o)
    save_npz(os.path.join(HERE, "g26_attn_block.npz"), **g26)

    # ---- G27 / G28: NCSNpp.forward at 768 x 64, scalar t and per-sample t -----------------------------------------
    for nf, name in ((8, "g27_ncsnpp_sgmse_nf8.npz"), (128, "g28_ncsnpp_sgmse_nf128.npz")):
        net = NCSNpp(nf=nf, **BB_SGMSE).eval()
        shapes = {"backbone." + k: list(v.shape) for k, v in net.state_dict().items()}
        sd = random_params(nf, shapes)
        net.load_state_dict(MG.to_t(MG.strip(sd, "backbone.")))
        x, y = forward_inputs(nf)
        g = dict(x_sum=checksum(x), y_sum=checksum(y), seed=np.int64(nf))
        for key, t in (("out_t025", [0.25]), ("out_t01_09", [0.1, 0.9])):
            o = net(torch.from_numpy(x), torch.from_numpy(y), torch.tensor(t)).numpy()
            g[key + "_s"] = sample(o)
            with bf16_rounding(net):
                ob = net(torch.from_numpy(x), torch.from_numpy(y), torch.tensor(t)).numpy()
            pred[f"{name[:3]}_{key}"] = rel(ob, o)
        save_npz(os.path.join(HERE, name), **g)
        print(name, os.path.getsize(os.path.join(HERE, name)) // 1024, "KiB", flush=True)

    # ---- G29: FlowModel.enhance of flow_model_sgmse (nf 128) on a 1 s clip, noise injected; ScoreModel PC at nf 8 ----
    sd128 = random_params(128, bb_shapes)
    fm.backbone.load_state_dict(MG.to_t(MG.strip(sd128, "backbone.")))
    y, noise = enhance_inputs()
    assert noise.shape[-1] == O.padded_frames(O.num_frames(y.shape[-1]))
    noise_t = torch.from_numpy(noise)
    fm._get_noise = lambda x, sigma: (sigma * noise_t[:x.shape[0]]).type(x.dtype)   # model.py:536
    g29 = dict(y_sum=checksum(y), noise_sum=checksum(noise), seed=np.int64(128))
    for solver, N in (("euler", 6), ("midpoint", 3)):
        xo = fm.enhance(torch.from_numpy(y), N=N, solver=solver).numpy()
        g29[f"{solver}_N{N}_s"] = sample(xo)
        with bf16_rounding(fm.backbone):
            xb = fm.enhance(torch.from_numpy(y), N=N, solver=solver).numpy()
        pred[f"g29_{solver}_N{N}"] = rel(xb, xo)
        print("g29", solver, N, pred[f"g29_{solver}_N{N}"], flush=True)
    # score_model_sgmse at nf 8 (output layer scaled down like G13), predictor-corrector sampler, seeded noise stream
    net8 = NCSNpp(nf=8, **BB_SGMSE)
    sd8 = random_params(8, {"backbone." + k: list(v.shape) for k, v in net8.state_dict().items()})
    sd8["backbone.output_layer.weight"] = (sd8["backbone.output_layer.weight"] * np.float32(SCORE_OUT_SCALE)).astype(np.float32)
    sm = ScoreModel(sde=OUVESDE(theta=1.5, sigma_min=0.05, sigma_max=0.5, N=30), t_eps=3e-2, backbone=net8, feature_extractor=fe,
                    sampling_rate=48000, lr=1e-4, full_config={}).eval()
    sm.backbone.load_state_dict(MG.to_t(MG.strip(sd8, "backbone.")))
    ys = score_input()
    Tps = O.padded_frames(O.num_frames(ys.shape[-1]))
    stream = O.seeded_noises(NOISE_SEED, (2, 1, 768, Tps))
    real = torch.randn_like
    torch.randn_like = lambda x, *a, **k: torch.from_numpy(next(stream))
    try:
        g29["score_y_sum"] = checksum(ys)
        g29["score_rd_ald_N3"] = sm.enhance(torch.from_numpy(ys), N=3, predictor="reverse_diffusion", corrector="ald", corrector_steps=1,
                                            snr=0.5).numpy()
    finally:
        torch.randn_like = real
    g29.update(score_noise_seed=np.int64(NOISE_SEED), score_out_scale=np.float64(SCORE_OUT_SCALE))
    save_npz(os.path.join(HERE, "g29_enhance_sgmse_nf128.npz"), **g29)
    print("g29", os.path.getsize(os.path.join(HERE, "g29_enhance_sgmse_nf128.npz")) // 1024, "KiB", flush=True)

    with open(os.path.join(HERE, "g30_sgmse_bf16_prediction.json"), "w") as f:
        json.dump(dict(model="reference with bf16 rounding of conv operands (input; weights except all_modules.3 and the Combine 1x1) "
                             "and of every stored module output; attention and output layer in f32 on stored tensors",
                       rel_l2=pred), f, indent=1)
    print(pred)


if __name__ == "__main__":
    main()
