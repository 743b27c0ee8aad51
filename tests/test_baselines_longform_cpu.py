"""Long-form and streaming for the ScoreDec and regression baselines: the surface that needs no GPU -- the four new C symbols and their
host-side refusals, the long-form hook of the three model classes, the refusals of the library and of the streaming pool, and the
command line of stream_cli."""
import ctypes as C
import inspect
import os
import re

import pytest

NEW = ("fd_score_enhance_chunks", "fd_regression_enhance_chunks", "fd_caxpy_at", "fd_score_update_at")


def test_symbols_header_and_bindings():
    from flowdec_amd import _lib
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "flowdec_hip.h")).read()
    lib = _lib.load()
    for name in NEW:
        assert re.search(r"^int %s\(" % name, header, re.M), f"{name} is not declared in the header"
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    # the bindings carry as many arguments as the declarations
    for name in NEW:
        decl = re.search(r"^int %s\((.*?)\);" % name, header, re.M | re.S).group(1)
        assert len(decl.split(",")) == len(_lib.SIGNATURES[name][1]), name
    # the signatures the existing callers use are unchanged: the *_at forms are additions
    assert len(_lib.SIGNATURES["fd_caxpy_at"][1]) == len(_lib.SIGNATURES["fd_op_caxpy"][1]) + 1
    assert len(_lib.SIGNATURES["fd_score_update_at"][1]) == len(_lib.SIGNATURES["fd_op_score_update"][1]) + 1
    assert "fd_score_enhance_chunks" in header.split("Seeded noise")[1].split("#define FD_NOISE_GAUSSIAN")[0], "the frame0 entry points of the noise contract"


def test_host_side_refusals_launch_nothing():
    """Every call below returns FD_EINVAL (-1) from its argument checks; the pointers are never dereferenced."""
    from flowdec_amd import _lib
    lib, p = _lib.load(), C.c_void_p(16)
    cfg = _lib.FdScoreConfig(1.5, 0.05, 0.5, 0.03, 0.5, 2, 0, 0, 1, 1)

    def refused(rc, word):
        assert rc == -1 and word in lib.fd_last_error().decode(), (rc, lib.fd_last_error())

    refused(lib.fd_score_enhance_chunks(None, p, p, p, None, None, C.byref(cfg), p, 1, 30000, p, 1 << 30, 0, None), "null model")
    refused(lib.fd_regression_enhance_chunks(None, p, p, None, p, 1, 30000, p, 1 << 30, 0, None), "null model")
    # caxpy: null pointers, a bad shape, no noise source, both, frame0 without seeds
    refused(lib.fd_caxpy_at(None, p, None, None, 0, 1.0, p, 1, 3, 64, None), "null pointer")
    refused(lib.fd_caxpy_at(p, p, None, None, 0, 1.0, None, 1, 3, 64, None), "null pointer")
    refused(lib.fd_caxpy_at(p, p, None, None, 0, 1.0, p, 0, 3, 64, None), "bad shape")
    refused(lib.fd_caxpy_at(p, None, None, None, 0, 1.0, p, 1, 3, 64, None), "exactly one")
    refused(lib.fd_caxpy_at(p, p, p, None, 0, 1.0, p, 1, 3, 64, None), "exactly one")
    refused(lib.fd_caxpy_at(p, None, p, None, -1, 1.0, p, 1, 3, 64, None), "draw")
    refused(lib.fd_caxpy_at(p, p, None, p, 0, 1.0, p, 1, 3, 64, None), "frame0 needs seeds")
    # score_update: the same, plus the image checks of fd_op_score_update
    tail = (p, 1, 3, 64, 1, _lib.FD_F32, None)
    refused(lib.fd_score_update_at(None, p, p, 1.0, p, 0.1, 0.2, p, None, None, 0, 0.3, *tail), "null pointer")
    refused(lib.fd_score_update_at(p, p, p, 1.0, None, 0.1, 0.2, p, None, None, 0, 0.3, *tail), "Y with cy")
    refused(lib.fd_score_update_at(p, p, p, 1.0, p, 0.1, 0.2, None, None, None, 0, 0.3, *tail), "exactly one")
    refused(lib.fd_score_update_at(p, p, p, 1.0, p, 0.1, 0.2, p, None, p, 0, 0.3, *tail), "frame0 needs seeds")
    refused(lib.fd_score_update_at(p, p, p, 1.0, p, 0.1, 0.2, None, None, p, 0, 0.0, *tail), "frame0 needs seeds")      # also with cz == 0
    refused(lib.fd_score_update_at(p, p, p, 1.0, p, 0.1, 0.2, p, None, None, 0, 0.3, p, 1, 3, 64, 2, _lib.FD_F32, None), "ks must be")
    assert "fd_score_update_at" in lib.fd_last_error().decode(), "the message names the entry point that was called"


def test_the_long_form_hook_of_the_three_classes():
    """One machinery in the base class, one hook per class; FlowModel's public surface is what it was."""
    import flowdec_amd
    from flowdec_amd import model as M
    classes = (flowdec_amd.FlowModel, flowdec_amd.ScoreModel, flowdec_amd.RegressionModel)
    for name in ("_enhance_long", "_enhance_long_rows", "_enhance_long_stitch", "_enhance_long_jobs", "_long_plan", "_long_stream", "_long_run_jobs",
                 "_long_stitch_rows", "_long_buffers"):
        assert name in vars(M._WaveModel) and all(name not in vars(c) for c in classes), name
    assert all("_chunks_call" in vars(c) for c in classes)
    E = inspect.Parameter.empty
    params = lambda f: [(k, p.default) for k, p in inspect.signature(f).parameters.items() if p.kind is not p.VAR_KEYWORD and k != "self"]
    assert params(M._WaveModel._enhance_long) == [("y", E), ("call", E), ("seed", None), ("row_frames", 3712), ("halo_frames", 256), ("xfade", None),
                                                  ("rows_per_call", 8), ("use_graph", True), ("normfac", None)]
    assert params(flowdec_amd.ScoreModel._chunks_call) == [("predictor", "reverse_diffusion"), ("corrector", "ald"), ("N", 30), ("corrector_steps", 1),
                                                           ("snr", 0.5), ("denoise", True), ("sampler_type", "pc"), ("eps", None), ("who", "enhance_long")]
    assert params(flowdec_amd.FlowModel._chunks_call) == [("N", 50), ("solver", "euler"), ("sigma_fac", 1.0), ("who", "enhance_long")]
    assert params(flowdec_amd.RegressionModel._chunks_call) == [("who", "enhance_long")]
    assert flowdec_amd.RegressionModel._draws_noise is False and flowdec_amd.ScoreModel._draws_noise is True
    want = dict(N=50, solver="euler", sigma_fac=1.0, seed=None, row_frames=3712, halo_frames=256, xfade=None, rows_per_call=8, use_graph=True)
    got = inspect.signature(flowdec_amd.FlowModel.enhance_long).parameters
    assert {k: p.default for k, p in got.items() if k not in ("self", "y")} == want


def test_library_refusals():
    import flowdec_amd
    from flowdec_amd.stream import EnhanceStream, StreamPool
    score = flowdec_amd.from_preset("baseline_scoredec_75s", nf=8)
    regr = flowdec_amd.from_preset("baseline_regression_75s", nf=8)
    flow = flowdec_amd.from_preset("flowdec_75m", nf=8)
    with pytest.raises(ValueError, match="'ode' sampler has no long-form"):
        score._chunks_call(sampler_type="ode")
    with pytest.raises(ValueError, match="unknown predictor"):
        score._chunks_call(predictor="heun")
    with pytest.raises(ValueError, match="unknown corrector"):
        score._chunks_call(corrector="langevin")
    with pytest.raises(ValueError, match="solver"):
        score._chunks_call(solver="euler")
    with pytest.raises(ValueError, match="no sampler arguments"):
        regr._chunks_call(N=2)
    with pytest.raises(ValueError, match="fixed-step"):
        flow._chunks_call(solver="dopri5")
    with pytest.raises(ValueError, match="predictor"):
        flow._chunks_call(predictor="none")
    assert callable(score._chunks_call(N=2, predictor="euler_maruyama", corrector="none")) and callable(regr._chunks_call())
    # the pool: a score model takes its sampler's arguments in place of `solver`
    with pytest.raises(ValueError, match="StreamPool.*solver"):
        StreamPool(score, solver="euler", normfac="causal")
    with pytest.raises(ValueError, match="StreamPool.*sigma_fac"):
        EnhanceStream(score, seed=1, sigma_fac=0.5, normfac="causal")
    with pytest.raises(ValueError, match="StreamPool.*'ode'"):
        StreamPool(score, sampler_type="ode", normfac="causal")
    with pytest.raises(ValueError, match="unknown predictor"):
        StreamPool(score, predictor="heun", normfac="causal")
    with pytest.raises(ValueError, match="StreamPool.*no sampler arguments"):
        StreamPool(regr, N=2, normfac="causal")
    # ... and the normalisation refusals hold for the two classes
    for m, kw in ((score, dict(N=2, predictor="none")), (regr, {})):
        assert m.normalize_mode == "noisy"
        with pytest.raises(ValueError, match="normfac"):
            StreamPool(m, normfac=None, **kw)
        for bad in ("peak", 0.0, -1.0, float("nan")):
            with pytest.raises(ValueError, match="normfac"):
                StreamPool(m, normfac=bad, **kw)
        with pytest.raises(ValueError, match="capacity"):
            StreamPool(m, capacity=0, normfac="causal", **kw)
        m.normalize_mode = "none"
        with pytest.raises(ValueError, match="normfac"):
            StreamPool(m, normfac=0.5, **kw)


def test_stream_cli_arguments(capsys):
    from flowdec_amd import stream_cli
    base = ["--ckpt", "m.ckpt", "--N", "6", "--seed", "7", "--normfac", "causal", "--format", "s16le"]
    a = stream_cli.parse_args(base)                                                   # today's argument lists parse unchanged
    assert (a.solver, a.row_frames, a.halo_frames, a.normfac, a.inp, a.out, a.block_samples) == ("euler", 256, 64, "causal", "-", "-", 4800)
    assert (a.predictor, a.corrector, a.corrector_steps, a.snr) == ("reverse_diffusion", "ald", 1, 0.5)
    a = stream_cli.parse_args(base + ["--predictor", "euler_maruyama", "--corrector", "none", "--corrector-steps", "3", "--snr", "0.33"])
    assert (a.predictor, a.corrector, a.corrector_steps, a.snr) == ("euler_maruyama", "none", 3, 0.33)
    a = stream_cli.parse_args(base + ["--solver", "midpoint", "--codes", "--codec", "w.pth"])
    assert a.solver == "midpoint" and a.codes

    def refused(argv, word):
        with pytest.raises(SystemExit) as e:
            stream_cli.parse_args(argv)
        assert e.value.code == 2 and word in capsys.readouterr().err

    refused([x for x in base if x not in ("--N", "6")], "--N")                          # what was required stays required
    refused([x for x in base if x not in ("--seed", "7")], "--seed")
    refused(base + ["--predictor", "heun"], "--predictor")
    refused(base + ["--corrector", "langevin"], "--corrector")
    refused(base + ["--corrector-steps", "-1"], "--corrector-steps")
    refused(base + ["--solver", "dopri5"], "--solver")
