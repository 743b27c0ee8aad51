"""Per-clip step control of the adaptive solvers, host side: the two new symbols, the CLI's batching rule, and the argument checks of
`enhance` / `enhance_batch` / `sharded_enhance`, all of which answer before a device is touched (the models here live on the CPU)."""
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BASE = ["--ckpt", "x.ckpt", "--files", "in", "--outdir", "out", "--N", "2"]


def test_symbols_are_declared_exported_and_bound():
    from flowdec_amd import _lib as L
    src = open(os.path.join(ROOT, "include", "flowdec_hip.h")).read()
    decl = set(re.findall(r"\b(fd_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", src, flags=re.S)))
    lib = L.load()
    for name in ("fd_ode_adaptive_clips_workspace_bytes", "fd_ode_solve_adaptive_clips"):
        assert name in decl, f"{name} is not declared in include/flowdec_hip.h"
        assert name in L.SIGNATURES, f"{name} has no ctypes signature"
        assert getattr(lib, name).argtypes == L.SIGNATURES[name][1]
    # (m, Y, noise, seeds, sigma_fac, N, method, atol, rtol, X_out, traj, nfe_out, rejected_out, evals_out, B, T_pad, ws, ws_bytes, stream)
    assert len(L.SIGNATURES["fd_ode_solve_adaptive_clips"][1]) == 19
    assert lib.fd_ode_adaptive_clips_workspace_bytes(None, 1, 64) == 0
    assert lib.fd_ode_solve_adaptive_clips(None, None, None, None, 1.0, 2, 0, 1e-3, 1e-3, None, None, None, None, None, 1, 64, None, 0, None) != 0
    assert b"null model" in lib.fd_last_error()


def test_cli_batches_an_adaptive_solver_only_with_step_control_clip():
    import flowdec_amd
    from flowdec_amd.enhance_cli import batchable, build_parser, enhance_kwargs
    flow = flowdec_amd.from_preset("flowdec_75m", nf=8)
    score = flowdec_amd.from_preset("baseline_scoredec_75s", nf=8)
    p = build_parser()
    assert p.parse_args(BASE).step_control == "batch"
    with pytest.raises(SystemExit):
        p.parse_args(BASE + ["--step-control", "file"])
    for solver in ("dopri5", "tsit5"):
        default, clip = p.parse_args(BASE + ["--solver", solver]), p.parse_args(BASE + ["--solver", solver, "--step-control", "clip"])
        assert not batchable(flow, default) and batchable(flow, clip)
        assert batchable(score, default) and batchable(score, clip)
        assert enhance_kwargs(flow, default) == dict(N=2, solver=solver)
        assert enhance_kwargs(flow, clip) == dict(N=2, solver=solver, step_control="clip")
        assert "step_control" not in enhance_kwargs(score, clip)
    # a fixed-step solver batches as before and never sees the keyword
    fixed = p.parse_args(BASE + ["--solver", "heun2", "--step-control", "clip"])
    assert batchable(flow, fixed) and enhance_kwargs(flow, fixed) == dict(N=2, solver="heun2")


def test_chunk_seconds_keeps_refusing_adaptive_solvers(tmp_path, capsys):
    from flowdec_amd import enhance_cli
    with pytest.raises(SystemExit):
        enhance_cli.run(["--ckpt", "x.ckpt", "--files", str(tmp_path), "--outdir", str(tmp_path / "o"), "--N", "2", "--solver", "dopri5",
                         "--step-control", "clip", "--chunk-seconds", "10", "--rng", "native"])
    assert "fixed-step" in capsys.readouterr().err


def test_value_errors_come_before_the_device():
    import flowdec_amd
    m = flowdec_amd.from_preset("flowdec_75m", nf=8)            # on the CPU: anything that gets past the checks says "GPU"
    y, clips = torch.zeros(1, 1, 12000), [torch.zeros(12000), torch.zeros(20000)]
    for solver in ("euler", "midpoint", "heun2", "heun2_eulerlast"):
        for sc in ("clip", "batch"):
            with pytest.raises(ValueError, match="step_control"):
                m.enhance(y, solver=solver, step_control=sc)
            with pytest.raises(ValueError, match="step_control"):
                m.enhance_batch(clips, solver=solver, step_control=sc)
    with pytest.raises(ValueError, match="step_control"):
        m.enhance(y, solver="dopri5", step_control="file")
    for solver in ("dopri5", "tsit5"):
        for sc in (None, "batch"):                               # a batch under ONE controller is not the one-by-one result: refused
            with pytest.raises(ValueError, match="step_control='clip'"):
                m.enhance_batch(clips, solver=solver, step_control=sc)
        with pytest.raises(ValueError, match="only one"):
            m.enhance_batch(clips, solver=solver, step_control="clip", seeds=[1, 2], generator=torch.Generator())
        with pytest.raises(RuntimeError, match="GPU"):
            m.enhance_batch(clips, solver=solver, step_control="clip", seeds=[1, 2])
        for sc in (None, "batch", "clip"):
            with pytest.raises(RuntimeError, match="GPU"):
                m.enhance(y, solver=solver, step_control=sc)
    with pytest.raises(ValueError, match="unknown solver"):
        m.enhance_batch(clips, solver="rk4", step_control="clip")


class _Recorder:
    """Stands in for a model in sharded_enhance: keeps the keywords of the enhance call."""
    device = torch.device("cpu")

    def __init__(self):
        self.kw = None

    def enhance(self, y, **kw):
        self.kw = kw
        return y


def test_sharded_enhance_forwards_step_control_on_both_noise_paths():
    from flowdec_amd.dist import sharded_enhance
    y = torch.zeros(3, 1, 12000)
    nz = torch.zeros(3, 1, 768, 64, dtype=torch.complex64)
    m = _Recorder()
    sharded_enhance(m, y, N=2, solver="dopri5", noise=nz, step_control="clip", atol=1e-2)
    assert m.kw["step_control"] == "clip" and m.kw["atol"] == 1e-2 and m.kw["noise"].shape == nz.shape
    sharded_enhance(m, y, N=2, solver="dopri5", seed=3, rng="native", step_control="clip")
    assert m.kw["step_control"] == "clip" and len(m.kw["seed"]) == 3
    sharded_enhance(m, y, N=2, solver="dopri5", noise=nz)          # unset: the keyword is not passed at all
    assert "step_control" not in m.kw
