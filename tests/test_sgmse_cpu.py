"""The SGMSE-style backbone (config/model/backbone/ncsnpp_default_ycond.yaml) on the host: native parameter layout, the module tree,
the presets and checkpoint loading against the reference's own state_dict manifest.  No GPU needed."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN

MANIFEST = json.load(open(os.path.join(GOLDEN, "state_dict_manifest_sgmse.json")))
BB_YAML = dict(image_size=768, nonlinearity="swish", nf=128, ch_mult=[1, 1, 2, 2, 2, 2, 2], num_res_blocks=2, attn_resolutions=[],
               bottleneck_attn=True, resamp_with_conv=True, conditional=True, fir=True, fir_kernel=[1, 3, 3, 1], skip_rescale=True,
               resblock_type="biggan", progressive="output_skip", progressive_input="input_skip", progressive_combine="sum",
               init_scale=0.0, embedding_type="fourier", fourier_scale=16, dropout=0.0, num_channels=4,
               output_layer_kwargs=dict(kernel_size=3, bias=False, padding="same", padding_mode="zeros"))


def backbone_manifest():
    return {k: v for k, v in MANIFEST.items() if k.startswith("backbone.")}


def lib():
    import __graft_entry__ as g
    g.build()
    from flowdec_amd import _lib
    return _lib, _lib.load()


def native_layout(cfg, arch):
    L, lb = lib()
    h = C.c_void_p()
    L.check(lb.fd_model_create_ex(C.byref(cfg), C.byref(arch), C.byref(h)))
    try:
        out = {}
        for i in range(lb.fd_model_num_params(h)):
            name, ndim, shape = C.c_char_p(), C.c_int(), (C.c_int * 4)()
            L.check(lb.fd_model_param_info(h, i, C.byref(name), C.byref(ndim), C.byref(shape)))
            out[name.value.decode()] = [shape[j] for j in range(ndim.value)]
        return out
    finally:
        lb.fd_model_destroy(h)


def sgmse_config(nf=128):
    L, _ = lib()
    cfg = L.FdModelConfig()
    cfg.nf = nf
    for i, c in enumerate((1, 1, 2, 2, 2, 2, 2)):
        cfg.ch_mult[i] = c
    cfg.num_levels, cfg.num_res_blocks, cfg.n_fft, cfg.hop, cfg.alpha, cfg.beta, cfg.act_dtype = 7, 2, 1534, 384, 0.5, 0.15, L.FD_BF16
    return cfg


def test_native_layout_is_the_reference_manifest():
    L, _ = lib()
    got = native_layout(sgmse_config(), L.FdModelArch(1, 3))
    ref = backbone_manifest()
    assert list(got) == list(ref)              # same order as the reference state_dict
    assert got == ref
    attn = [k for k in got if ".NIN_" in k or k.endswith("all_modules.31.GroupNorm_0.weight")]
    assert len(attn) == 9 and all(k.startswith("backbone.all_modules.31.") for k in attn)
    assert got["backbone.output_layer.weight"] == [2, 4, 3, 3]


def test_create_ex_defaults_and_limits():
    L, lb = lib()
    # fd_model_create == fd_model_create_ex with {0, 1}: the shipped layout is unchanged
    cfg = sgmse_config(64)
    for i, c in enumerate((4, 4, 4, 2)):
        cfg.ch_mult[i] = c
    cfg.num_levels, cfg.num_res_blocks = 4, 1
    h = C.c_void_p()
    L.check(lb.fd_model_create(C.byref(cfg), C.byref(h)))
    n = lb.fd_model_num_params(h)
    lb.fd_model_destroy(h)
    assert list(native_layout(cfg, L.FdModelArch(0, 1))) == list(native_layout(cfg, L.FdModelArch(0, 1)))
    assert len(native_layout(cfg, L.FdModelArch(0, 1))) == n
    # nf 128 is accepted now; nf 12 (not a multiple of 8) and nf 136 are not
    assert native_layout(sgmse_config(128), L.FdModelArch(1, 3))
    for nf in (12, 136):
        h = C.c_void_p()
        assert lb.fd_model_create_ex(C.byref(sgmse_config(nf)), C.byref(L.FdModelArch(1, 3)), C.byref(h)) != 0
        assert b"nf" in lb.fd_last_error()
    for arch in ((0, 2), (2, 1), (1, 5)):
        h = C.c_void_p()
        assert lb.fd_model_create_ex(C.byref(sgmse_config(128)), C.byref(L.FdModelArch(*arch)), C.byref(h)) != 0


def test_ncsnpp_module_tree_matches_manifest():
    from flowdec_amd.model import NCSNpp
    kw = {k: tuple(v) if isinstance(v, list) else v for k, v in BB_YAML.items()}
    net = NCSNpp(**kw)
    got = {"backbone." + k: list(v.shape) for k, v in net.state_dict().items()}
    ref = backbone_manifest()
    assert list(got) == list(ref) and got == ref
    assert net.bottleneck_attn and net.output_ksize == 3
    # padding given as an integer is the same layer
    kw["output_layer_kwargs"] = dict(kernel_size=3, bias=False, padding=1)
    assert list(NCSNpp(**kw).state_dict()) == list(net.state_dict())


def test_unsupported_attention_and_output_layers_still_raise():
    from flowdec_amd.model import NCSNpp
    kw = {k: tuple(v) if isinstance(v, list) else v for k, v in BB_YAML.items()}
    for bad in (dict(attn_resolutions=(768,)), dict(attn_resolutions=(24,)),
                dict(output_layer_kwargs=dict(kernel_size=3, bias=True, padding="same")),
                dict(output_layer_kwargs=dict(kernel_size=3, bias=False, padding=0)),
                dict(output_layer_kwargs=dict(kernel_size=3, bias=False, padding="same", padding_mode="reflect")),
                dict(output_layer_kwargs=dict(kernel_size=5, bias=False, padding="same"))):
        with pytest.raises(NotImplementedError):
            NCSNpp(**{**kw, **bad})


def test_presets():
    import flowdec_amd
    from flowdec_amd.model import FlowModel, ScoreModel
    fm = flowdec_amd.from_preset("flow_model_sgmse")
    assert isinstance(fm, FlowModel)
    assert fm.backbone.nf == 128 and fm.backbone.num_res_blocks == 2 and fm.backbone.bottleneck_attn and fm.backbone.output_ksize == 3
    assert fm.backbone.ch_mult == (1, 1, 2, 2, 2, 2, 2)
    assert fm.feature_extractor._cfg() == dict(n_fft=1534, hop=384, alpha=0.5, beta=0.15)
    assert fm.sigma_y.numel() == 1 and float(fm.sigma_y) == 0.5
    assert {"backbone." + k: list(v.shape) for k, v in fm.backbone.state_dict().items()} == backbone_manifest()
    sm = flowdec_amd.from_preset("score_model_sgmse", nf=8)
    assert isinstance(sm, ScoreModel) and sm.backbone.nf == 8 and sm.backbone.bottleneck_attn
    assert (sm.sde.theta, sm.sde.sigma_min, sm.sde.sigma_max, sm.sde.N, sm.t_eps) == (1.5, 0.05, 0.5, 30, 3e-2)
    assert sm.feature_extractor._cfg()["alpha"] == 0.5 and sm.feature_extractor._cfg()["beta"] == 0.15
    # the shipped presets are untouched
    f75 = flowdec_amd.from_preset("flowdec_75m", nf=8)
    assert not f75.backbone.bottleneck_attn and f75.backbone.output_ksize == 1 and f75.feature_extractor._cfg()["alpha"] == 0.3


def test_model_from_checkpoint_sgmse():
    from flowdec_amd.enhance_cli import model_from_checkpoint
    sd = {k: torch.full(tuple(v), 0.01) for k, v in MANIFEST.items()}
    hp = {"model": {"_target_": "flowdec.model.FlowModel", "sigma_x": 0.0, "sigma_y": 0.5,
                    "backbone": {"_target_": "flowdec.backbones.ncsnpp.NCSNpp", **BB_YAML},
                    "feature_extractor": {"_target_": "flowdec.data.feature_extractors.AmplitudeCompressedComplexSTFT", "n_fft": 1534,
                                          "n_hops": 4, "window_fn": "hann", "sampling_rate": 48000, "alpha": 0.5, "beta": 0.15}},
          "sampling_rate": 48000}
    ckpt = {"state_dict": sd, "_pl_ema_state_dict": sd, "hyper_parameters": hp}
    m = model_from_checkpoint(ckpt, ema=True, precision="fp32")
    res = m.load_state_dict(sd, strict=False)
    assert not [k for k in res.missing_keys if k.startswith("backbone.")]
    assert not [k for k in res.unexpected_keys if k.startswith("backbone.")]
    assert m.backbone.nf == 128 and m.backbone.bottleneck_attn and m.backbone.output_ksize == 3
    assert float(m.backbone.all_modules[31].NIN_2.W[0, 0]) == pytest.approx(0.01)
    assert m.feature_extractor._cfg()["alpha"] == 0.5


def test_golden_weight_generator_covers_the_layout():
    """The seeded weights the GPU tests load come from tests/golden/make_golden_sgmse.py on the manifest's layout."""
    import importlib.util as ilu
    spec = ilu.spec_from_file_location("_mg_sgmse", os.path.join(GOLDEN, "make_golden_sgmse.py"))
    gen = ilu.module_from_spec(spec); spec.loader.exec_module(gen)
    sd = gen.random_params(128, backbone_manifest())
    assert list(sd) == list(backbone_manifest())
    assert all(list(v.shape) == backbone_manifest()[k] and v.dtype == np.float32 for k, v in sd.items())
    assert abs(float(np.std(sd["backbone.all_modules.31.NIN_0.W"])) - 1 / 16) < 5e-3
