"""(CPU) The command line runs every model class the reference's `enhance.py` can load (enhance.py:66): the checkpoint reader builds
the class `hyper_parameters.model._target_` names, the score model's SDE comes from the checkpoint, the sampler flags reach the model,
and the two ragged entry points of the baselines (fd_score_enhance_ragged, fd_regression_enhance_ragged) are exported and refuse bad
arguments on the host."""
import ctypes as C
import os
import re
from collections.abc import Mapping, Sequence

import pytest

from conftest import ROOT
from test_cli import synthetic_ckpt

FD_EINVAL = -1
BASE = ["--ckpt", "a", "--files", "b", "--outdir", "c"]
# values that differ from config/model/sde/ouve_final.yaml (1.5, 0.05, 0.82, 30) and score_model_final.yaml (t_eps 3e-2): a reader that
# fell back to the defaults fails
SDE = {"_target_": "flowdec.sdes.OUVESDE", "theta": 2.25, "sigma_min": 0.07, "sigma_max": 0.61, "N": 17}
T_EPS = 0.045


class _FakeDictConfig(Mapping):
    """Stands in for omegaconf.DictConfig (see test_cli._FakeDictConfig): a Mapping that is not a dict, nested nodes of the same kind."""

    def __init__(self, d):
        self._d = {k: (_FakeDictConfig(v) if isinstance(v, dict) else (_FakeList(v) if isinstance(v, list) else v)) for k, v in d.items()}

    def __getitem__(self, k): return self._d[k]
    def __iter__(self): return iter(self._d)
    def __len__(self): return len(self._d)


class _FakeList(Sequence):
    def __init__(self, v): self._v = list(v)
    def __getitem__(self, i): return self._v[i]
    def __len__(self): return len(self._v)


def ckpt_of(target=None, sde=None, t_eps=None, wrap=False):
    ckpt = synthetic_ckpt()
    m = ckpt["hyper_parameters"]["model"]
    if target is not None:
        m["_target_"] = target
    if sde is not None:
        m["sde"] = dict(sde)
    if t_eps is not None:
        m["t_eps"] = t_eps
    if wrap:
        ckpt["hyper_parameters"] = _FakeDictConfig(ckpt["hyper_parameters"])
    return ckpt


@pytest.mark.parametrize("wrap", [False, True], ids=["dict", "dictconfig"])
def test_checkpoint_names_the_model_class(wrap):
    from flowdec_amd import FlowModel, RegressionModel, ScoreModel
    from flowdec_amd.enhance_cli import model_from_checkpoint
    m = model_from_checkpoint(ckpt_of("flowdec.model.ScoreModel", SDE, T_EPS, wrap))
    assert type(m) is ScoreModel and m.backbone.nf == 8 and not m.training
    assert (m.sde.theta, m.sde.sigma_min, m.sde.sigma_max, m.sde.N, m.t_eps) == (2.25, 0.07, 0.61, 17, T_EPS)
    m = model_from_checkpoint(ckpt_of("flowdec.model.RegressionModel", wrap=wrap))
    assert type(m) is RegressionModel and m.backbone.nf == 8
    assert type(model_from_checkpoint(ckpt_of("flowdec.model.FlowModel", wrap=wrap))) is FlowModel
    assert type(model_from_checkpoint(ckpt_of(wrap=wrap))) is FlowModel               # no _target_: a FlowModel, as before
    # --model overrides the checkpoint, in both directions
    assert type(model_from_checkpoint(ckpt_of("flowdec.model.ScoreModel", SDE, T_EPS, wrap), model="regression")) is RegressionModel
    m = model_from_checkpoint(ckpt_of("flowdec.model.FlowModel", SDE, T_EPS, wrap), model="score")
    assert type(m) is ScoreModel and m.sde.theta == 2.25 and m.t_eps == T_EPS
    with pytest.raises(RuntimeError, match="VeryNewModel"):
        model_from_checkpoint(ckpt_of("flowdec.model.VeryNewModel", wrap=wrap))
    for sde in ("OUVPSDE", "BBEDSDE"):
        with pytest.raises(RuntimeError, match=sde):
            model_from_checkpoint(ckpt_of("flowdec.model.ScoreModel", dict(SDE, _target_=f"flowdec.sdes.{sde}"), T_EPS, wrap))
    # the score model reads the EMA weights like the flow model does
    raw = model_from_checkpoint(ckpt_of("flowdec.model.ScoreModel", SDE, T_EPS, wrap), ema=False)
    ema = model_from_checkpoint(ckpt_of("flowdec.model.ScoreModel", SDE, T_EPS, wrap), ema=True)
    key = "backbone.all_modules.3.bias"
    assert (ema.state_dict()[key] - raw.state_dict()[key] - 1.0).abs().max() < 1e-6


def test_bare_state_dict_and_model_flag():
    from flowdec_amd import FlowModel, RegressionModel, ScoreModel
    from flowdec_amd.enhance_cli import model_from_checkpoint
    sd = synthetic_ckpt()["_pl_ema_state_dict"]
    assert type(model_from_checkpoint(sd)) is FlowModel
    assert type(model_from_checkpoint(synthetic_ckpt(with_hp=False))) is FlowModel
    assert type(model_from_checkpoint(sd, model="flow")) is FlowModel
    m = model_from_checkpoint(sd, model="score")      # config/model/sde/ouve_final.yaml + score_model_final.yaml's t_eps
    assert type(m) is ScoreModel and m.backbone.nf == 8
    assert (m.sde.theta, m.sde.sigma_min, m.sde.sigma_max, m.sde.N, m.t_eps) == (1.5, 0.05, 0.82, 30, 3e-2)
    assert type(model_from_checkpoint(sd, model="regression")) is RegressionModel
    with pytest.raises(ValueError):
        model_from_checkpoint(sd, model="bogus")
    # a score checkpoint that names its class but carries no sde / t_eps gets the same defaults
    m = model_from_checkpoint(ckpt_of("flowdec.model.ScoreModel"))
    assert (m.sde.theta, m.sde.sigma_min, m.sde.sigma_max, m.sde.N, m.t_eps) == (1.5, 0.05, 0.82, 30, 3e-2)


def test_load_from_checkpoint_takes_model(tmp_path):
    import torch
    from flowdec_amd import RegressionModel, ScoreModel
    from flowdec_amd.enhance_cli import load_from_checkpoint
    torch.save(ckpt_of("flowdec.model.ScoreModel", SDE, T_EPS), tmp_path / "s.ckpt")
    assert type(load_from_checkpoint(str(tmp_path / "s.ckpt"))) is ScoreModel
    assert type(load_from_checkpoint(str(tmp_path / "s.ckpt"), model="regression")) is RegressionModel


def test_parser_flags():
    from flowdec_amd.enhance_cli import build_parser
    p = build_parser()
    a = p.parse_args(BASE + ["--N", "1"])
    assert (a.model, a.predictor, a.corrector, a.snr) == ("auto", "reverse_diffusion", "ald", 0.5)
    for kind in ("auto", "flow", "score", "regression"):
        assert p.parse_args(BASE + ["--N", "1", "--model", kind]).model == kind
    assert p.parse_args(BASE + ["--N", "1", "--predictor", "euler_maruyama", "--corrector", "none"]).corrector == "none"
    for bad in (["--predictor", "bogus"], ["--corrector", "bogus"], ["--model", "bogus"]):
        with pytest.raises(SystemExit):
            p.parse_args(BASE + ["--N", "1"] + bad)


def test_keyword_builder_per_model_class():
    import flowdec_amd
    from flowdec_amd.enhance_cli import batchable, build_parser, enhance_kwargs, noise_kwargs
    args = build_parser().parse_args(BASE + ["--N", "4", "--predictor", "euler_maruyama", "--corrector", "none", "--snr", "0.3", "--solver", "heun2",
                                             "--rng", "native", "--seed", "5"])
    score = flowdec_amd.from_preset("baseline_scoredec_75s", nf=8)
    flow = flowdec_amd.from_preset("flowdec_75m", nf=8)
    reg = flowdec_amd.from_preset("baseline_regression_75s", nf=8)
    assert enhance_kwargs(score, args) == dict(N=4, predictor="euler_maruyama", corrector="none", snr=0.3)
    assert enhance_kwargs(flow, args) == dict(N=4, solver="heun2")
    assert enhance_kwargs(reg, args) == {}
    # the regression model draws no noise: --seed / --rng are accepted and ignored; the other two get one seed per file
    assert noise_kwargs(reg, args, [0, 1], batch=True) == {} and noise_kwargs(reg, args, [0], batch=False) == {}
    from flowdec_amd.noise import clip_seed
    assert noise_kwargs(score, args, [2, 3], batch=True) == dict(seeds=[clip_seed(5, 2), clip_seed(5, 3)])
    assert noise_kwargs(score, args, [2], batch=False) == dict(seed=[clip_seed(5, 2)])
    # the adaptive solvers keep a flow model out of batches; the baselines ignore --solver
    args.solver = "dopri5"
    assert not batchable(flow, args) and batchable(score, args) and batchable(reg, args)


def test_enhance_batch_rejects_what_it_cannot_run_before_touching_a_device():
    import torch
    import flowdec_amd
    s = flowdec_amd.from_preset("baseline_scoredec_75s", nf=8)
    y = [torch.zeros(12000), torch.zeros(20000)]
    with pytest.raises(ValueError, match="ode"):
        s.enhance_batch(y, sampler_type="ode")
    with pytest.raises(ValueError, match="only one"):
        s.enhance_batch(y, seeds=[1, 2], generator=torch.Generator())
    with pytest.raises(ValueError, match="predictor"):
        s.enhance_batch(y, predictor="bogus")
    with pytest.raises(RuntimeError, match="GPU"):           # no CPU compute path
        s.enhance_batch(y, N=1)
    with pytest.raises(RuntimeError, match="GPU"):
        flowdec_amd.from_preset("baseline_regression_75s", nf=8).enhance_batch(y)


def _host_model(lib, L):
    cfg = L.FdModelConfig()
    cfg.nf, cfg.num_levels, cfg.num_res_blocks, cfg.n_fft, cfg.hop, cfg.act_dtype = 8, 4, 1, 1534, 384, 1
    cfg.alpha, cfg.beta = 0.3, 0.33
    for i, c in enumerate((4, 4, 4, 2)):
        cfg.ch_mult[i] = c
    h = C.c_void_p()
    assert lib.fd_model_create(C.byref(cfg), C.byref(h)) == 0
    return h


def test_ragged_symbols_and_host_side_refusals():
    from flowdec_amd import _lib as L
    src = open(os.path.join(ROOT, "include", "flowdec_hip.h")).read()
    decl = set(re.findall(r"\b(fd_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", src, flags=re.S)))
    lib = L.load()
    for name in ("fd_score_enhance_ragged", "fd_regression_enhance_ragged"):
        assert name in decl, f"{name} is not declared in include/flowdec_hip.h"
        assert name in L.SIGNATURES, f"{name} has no ctypes signature"
        assert hasattr(lib, name), f"{name} is not exported"
    # argument errors are answered on the host, before the model's state is looked at: a model that was never finalized (no device needed)
    # and pointers that are never dereferenced
    h = _host_model(lib, L)
    p = C.c_void_p(256)
    ok = L.FdScoreConfig(1.5, 0.05, 0.82, 0.03, 0.5, 3, 0, 0, 1, 1)

    def score(lengths=p, noise=None, seeds=None, cfg=ok, B=2):
        return lib.fd_score_enhance_ragged(h, p, lengths, noise, seeds, C.byref(cfg), p, B, 24575, p, 1 << 40, 0, None)

    for kw, why in ((dict(noise=p, seeds=p), b"exactly one of noise and seeds"), (dict(), b"exactly one of noise and seeds"),
                    (dict(lengths=None, seeds=p), b"null lengths"), (dict(seeds=p, B=0), b"B must be positive"),
                    (dict(noise=p, B=-3), b"B must be positive"),
                    (dict(seeds=p, cfg=L.FdScoreConfig(1.5, 0.05, 0.82, 0.03, 0.5, 3, 7, 0, 1, 1)), b"unknown predictor id 7"),
                    (dict(seeds=p, cfg=L.FdScoreConfig(1.5, 0.05, 0.82, 0.03, 0.5, 3, 0, 5, 1, 1)), b"unknown corrector id 5")):
        assert score(**kw) == FD_EINVAL and why in lib.fd_last_error(), (kw, lib.fd_last_error())
    assert b"both" in (score(noise=p, seeds=p), lib.fd_last_error())[1] and b"neither" in (score(), lib.fd_last_error())[1]
    assert lib.fd_regression_enhance_ragged(h, p, None, p, 2, 24575, p, 1 << 40, 0, None) == FD_EINVAL and b"null lengths" in lib.fd_last_error()
    assert lib.fd_regression_enhance_ragged(h, p, p, p, 0, 24575, p, 1 << 40, 0, None) == FD_EINVAL and b"B must be positive" in lib.fd_last_error()
    assert lib.fd_score_enhance_ragged(None, p, p, None, p, C.byref(ok), p, 2, 24575, p, 1 << 40, 0, None) == FD_EINVAL
    # a well-formed call on this model gets as far as the model's own state: it was never finalized
    assert score(seeds=p) != 0 and b"exactly one" not in lib.fd_last_error() and b"null" not in lib.fd_last_error()
    lib.fd_model_destroy(h)
