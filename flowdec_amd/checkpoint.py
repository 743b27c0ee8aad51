"""Reads a Lightning checkpoint (or a bare state_dict) into the model class it names: the replacement of
`EnhancementModel.load_from_checkpoint` (enhance.py:66) that every command line of the package loads its model with.

Checkpoints: a Lightning `.ckpt` (dict with `_pl_ema_state_dict` and/or `state_dict`, optionally `hyper_parameters`
holding the resolved config: callbacks/ema.py:201-215, model.py:100,119) or a bare state_dict.  `ema=True` (the default)
selects the EMA weights exactly like `demo.ipynb` cell 2.  The class is the one `hyper_parameters.model._target_` names --
FlowModel, ScoreModel or RegressionModel; a checkpoint that names none is a FlowModel (`model_kind`).
"""
from typing import Tuple

import torch

from .model import (BACKBONE_FINAL_NO_ATTN, OUVESDE, PRESETS, AmplitudeCompressedComplexSTFT, FlowModel, NCSNpp, RegressionModel, ScoreModel,
                    from_preset)


def _to_plain(obj):
    """hyper_parameters of a real Lightning checkpoint are an OmegaConf DictConfig (the reference calls
    save_hyperparameters(self.full_config), model.py:60-63), not a dict: convert any Mapping / sequence tree to plain
    Python containers (OmegaConf.to_container when omegaconf is importable, so that interpolations are resolved)."""
    from collections.abc import Mapping, Sequence
    try:
        from omegaconf import OmegaConf
        if OmegaConf.is_config(obj):
            return OmegaConf.to_container(obj, resolve=True)
    except ImportError:
        pass
    if isinstance(obj, Mapping):
        return {k: _to_plain(v) for k, v in obj.items()}
    if isinstance(obj, Sequence) and not isinstance(obj, (str, bytes)):
        return [_to_plain(v) for v in obj]
    return obj


def _cfg_get(cfg, *path, default=None):
    for k in path:
        if isinstance(cfg, dict) and k in cfg:
            cfg = cfg[k]
        else:
            return default
    return cfg


MODEL_KINDS = {"flow": FlowModel, "score": ScoreModel, "regression": RegressionModel}


def model_kind(mcfg: dict, model: str = "auto") -> str:
    """'flow' / 'score' / 'regression': `model` unless it is 'auto', else the class `hyper_parameters.model._target_` names (the class
    EnhancementModel.load_from_checkpoint would build, enhance.py:66); a checkpoint without a `_target_` is a FlowModel."""
    if model != "auto":
        if model not in MODEL_KINDS:
            raise ValueError(f"model must be one of {['auto'] + sorted(MODEL_KINDS)} (got {model!r})")
        return model
    target = mcfg.get("_target_")
    if target is None:
        return "flow"
    for kind, cls in MODEL_KINDS.items():
        if str(target).split(".")[-1] == cls.__name__:
            return kind
    raise RuntimeError(f"checkpoint names the model class {target!r}: only FlowModel, ScoreModel and RegressionModel are implemented "
                       f"(--model overrides the checkpoint)")


def score_settings(mcfg: dict) -> Tuple[OUVESDE, float]:
    """(sde, t_eps) of a ScoreModel checkpoint: `model.sde` (theta, sigma_min, sigma_max, N) and `model.t_eps`; what is absent comes from
    config/model/sde/ouve_final.yaml and score_model_final.yaml's t_eps (the preset baseline_scoredec_75s).  Only the OUVE SDE exists here."""
    default = PRESETS["baseline_scoredec_75s"]
    sde_cfg = mcfg.get("sde") or {}
    target = sde_cfg.get("_target_")
    if target is not None and str(target).split(".")[-1] != "OUVESDE":
        raise RuntimeError(f"checkpoint names the SDE {target!r}: only OUVESDE is implemented")
    par = {k: sde_cfg.get(k, v) for k, v in default["sde"].items()}
    t_eps = mcfg.get("t_eps")
    return OUVESDE(**par), float(default["t_eps"] if t_eps is None else t_eps)


def model_from_checkpoint(ckpt, ema: bool = True, precision: str = "bf16", preset: str = "flowdec_75m", model: str = "auto"):
    """Build the FlowModel, ScoreModel or RegressionModel of a loaded checkpoint object (see module docstring for the accepted layouts
    and `model_kind` for the choice of the class)."""
    if not isinstance(ckpt, dict):
        raise RuntimeError("checkpoint must be a dict")
    if "_pl_ema_state_dict" in ckpt or "state_dict" in ckpt:
        key = "_pl_ema_state_dict" if (ema and "_pl_ema_state_dict" in ckpt) else "state_dict"
        if key not in ckpt:
            raise RuntimeError(f"checkpoint has no '{key}' (available: {[k for k in ckpt if 'state_dict' in k]})")
        sd = ckpt[key]
    else:
        sd = ckpt  # bare state_dict
    hp = None
    if ckpt.get("hyper_parameters", None) is not None:
        hp = _to_plain(ckpt["hyper_parameters"])
        if not isinstance(hp, dict):   # silently falling back to the defaults would produce wrong audio for e.g. the ablation configs
            raise RuntimeError(f"checkpoint 'hyper_parameters' of type {type(ckpt['hyper_parameters']).__name__} cannot be read as a mapping")
    mcfg = _cfg_get(hp, "model") or {}
    bb_cfg = dict(BACKBONE_FINAL_NO_ATTN)
    for k, v in (mcfg.get("backbone") or {}).items():
        if k != "_target_":
            bb_cfg[k] = tuple(v) if isinstance(v, list) else v
    if not mcfg.get("backbone") and "backbone.all_modules.0.W" in sd:      # infer the width from the weights
        bb_cfg["nf"] = int(sd["backbone.all_modules.0.W"].shape[0])
    fe_cfg = mcfg.get("feature_extractor") or {}
    fe = AmplitudeCompressedComplexSTFT(window_fn=fe_cfg.get("window_fn", "hann"), n_fft=int(fe_cfg.get("n_fft", 1534)),
                                        n_hops=int(fe_cfg.get("n_hops", 4)) if "hop_length" not in fe_cfg else None,
                                        hop_length=fe_cfg.get("hop_length"), sampling_rate=int(_cfg_get(hp, "sampling_rate", default=48000)),
                                        alpha=float(fe_cfg.get("alpha", 0.3)), beta=float(fe_cfg.get("beta", 0.33)))
    kind = model_kind(mcfg, model)
    common = dict(backbone=NCSNpp(precision=precision, **bb_cfg), feature_extractor=fe, sampling_rate=int(_cfg_get(hp, "sampling_rate", default=48000)))
    if kind == "score":
        sde, t_eps = score_settings(mcfg)
        net = ScoreModel(sde=sde, t_eps=t_eps, **common)
    elif kind == "regression":
        net = RegressionModel(**common)
    else:
        sigma_y = sd["sigma_y"] if "sigma_y" in sd else from_preset(preset, nf=8).sigma_y.data
        net = FlowModel(sigma_x=0.0, sigma_y=sigma_y.clone(), **common)
    res = net.load_state_dict(sd, strict=False)  # strict_loading = False in the reference (model.py:397)
    missing = [k for k in res.missing_keys if k.startswith("backbone.")]
    if missing:
        raise RuntimeError(f"checkpoint is missing backbone parameters, e.g. {missing[:3]}")
    return net.eval()


def load_from_checkpoint(path: str, map_location="cpu", ema: bool = True, precision: str = "bf16", model: str = "auto"):
    """Replacement for `EnhancementModel.load_from_checkpoint(ckpt, map_location=..., ema=...)` (enhance.py:66)."""
    ckpt = torch.load(path, map_location="cpu", weights_only=False)
    net = model_from_checkpoint(ckpt, ema=ema, precision=precision, model=model)
    return net.to(map_location) if map_location is not None else net
