"""The ScoreDec ODE sampler's device driver, the parts that need no GPU: the step-size controller Rk45Ctl (flowdec_amd/csrc/step_ctl.h)
against scipy.integrate.RK45 itself, the argument errors of the Python entry points, and the command line's --sampler switch.

tests/c/rk45_ctl_check.cpp includes the header directly, has its own main and is built twice with g++ -std=c++17: plain, and with
-fsanitize=address,undefined -fno-sanitize-recover=all; it runs as a stand-alone executable."""
import os
import shutil
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
BUILDS = {"plain": [], "sanitized": ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}
THETA, SIGMA_MIN, SIGMA_MAX, EPS = 1.5, 0.05, 0.5, 0.03
BASE = ["--ckpt", "x.ckpt", "--files", "in", "--outdir", "out", "--N", "2"]


@pytest.fixture(scope="module", params=sorted(BUILDS))
def rk45_ctl(request, tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path_factory.mktemp("rk45_" + request.param) / "rk45_ctl_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", *BUILDS[request.param], "-I", os.path.join(ROOT, "flowdec_amd", "csrc"),
                    "-I", os.path.join(ROOT, "include"), os.path.join(HERE, "c", "rk45_ctl_check.cpp"), "-o", exe], check=True)
    return exe


def run(exe, *args):
    r = subprocess.run([exe, *[repr(float(a)) for a in args]], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    return [dict(kind=t[0], **dict(zip(t[1::2], t[2::2]))) for t in (line.split() for line in r.stdout.splitlines())]


def pf_ode():
    """The OUVE probability-flow ODE of point-mass data x0 seen through y, 16 complex elements: score = -(x - mu_t) / std_t^2 in closed
    form, so the drift is theta (y - x) - g^2 / 2 score.  -> (fun(t, x), x_T complex64)."""
    rng = np.random.default_rng(0)
    cplx = lambda: rng.standard_normal(16) + 1j * rng.standard_normal(16)
    x0, y, z = cplx(), cplx(), cplx()
    ls = np.log(SIGMA_MAX / SIGMA_MIN)
    std = lambda t: np.sqrt(SIGMA_MIN ** 2 * np.exp(-2 * THETA * t) * (np.exp(2 * (THETA + ls) * t) - 1) * ls / (THETA + ls))
    g = lambda t: SIGMA_MIN * (SIGMA_MAX / SIGMA_MIN) ** t * np.sqrt(2 * ls)

    def fun(t, x):
        mu = np.exp(-THETA * t) * x0 + (1 - np.exp(-THETA * t)) * y
        return THETA * (y - x) + 0.5 * g(t) ** 2 * (x - mu) / std(t) ** 2
    return fun, (y + std(1.0) * z).astype(np.complex64)


@pytest.mark.parametrize("tol", [1e-3, 1e-5])
def test_controller_equals_scipy_rk45(rk45_ctl, tol):
    """Rk45Ctl fed scipy's own error norms takes scipy's steps: the first step equals select_initial_step's, every t and h of every
    attempt equals scipy's as a double (no tolerance: this libm's pow agrees with numpy's on these traces), accept flags and the attempt
    count are exact.  The traces are live: each holds a rejected attempt, an accepted attempt right after a rejection (the branch
    that caps the growth factor at 1), and ends on the clamp to eps."""
    from scipy.integrate import RK45
    from scipy.integrate._ivp.common import norm
    fun, xT = pf_ode()
    s = RK45(fun, 1.0, xT, EPS, rtol=tol, atol=tol)
    # select_initial_step's three norms, by its own formula (scipy/integrate/_ivp/common.py)
    y0, f0 = s.y, s.f
    scale = tol + np.abs(y0) * tol
    d0, d1 = norm(y0 / scale), norm(f0 / scale)
    h0 = min(1e-6 if d0 < 1e-5 or d1 < 1e-5 else 0.01 * d0 / d1, abs(EPS - 1.0))
    d2 = norm((fun(1.0 - h0, y0 - h0 * f0) - f0) / scale) / h0
    first = s.h_abs
    rec = []   # per attempt: t at its start, the signed step, scipy's norm
    inner = s._estimate_error_norm

    def spy(K, h, scale):
        e = inner(K, h, scale)
        rec.append((float(s.t), float(h), float(e)))
        return e
    s._estimate_error_norm = spy
    after = {}   # attempt index of an accepted step -> (t, h_abs) after it
    while s.status == "running":
        assert s.step() is None
        after[len(rec) - 1] = (float(s.t), float(s.h_abs))
    assert s.status == "finished" and s.nfev == 2 + 6 * len(rec)
    out = run(rk45_ctl, 1.0, EPS, d0, d1, d2, *[e for _, _, e in rec])
    assert out[0]["kind"] == "probe" and float(out[0]["h0"]) == h0 and float(out[0]["t"]) == 1.0 - h0
    assert out[1]["kind"] == "first" and float(out[1]["h_abs"]) == first
    tries = out[2:-1]
    assert [a["kind"] for a in tries] == ["attempt"] * len(rec)
    assert (out[-1]["kind"], out[-1]["attempts"], float(out[-1]["t"])) == ("done", str(len(rec)), EPS)
    for i, (a, (t, h, e)) in enumerate(zip(tries, rec)):
        assert float(a["t"]) == t and float(a["h"]) == h, (i, a, t, h)
        assert a["accept"] == ("1" if e < 1 else "0"), (i, a, e)
        assert (a["accept"] == "1") == (i in after)
        if i in after:
            assert (float(a["t_new"]), float(a["h_abs"])) == after[i], (i, a, after[i])
    flags = "".join(a["accept"] for a in tries)
    assert "0" in flags and "01" in flags, flags   # (this problem: 7 attempts, 2 rejected at 1e-3; 11 and 3 at 1e-5)
    last = tries[-1]
    assert float(last["t_new"]) == EPS and abs(float(last["h"])) < float(tries[-2]["h_abs"]), "the last step is not the clamp to eps"


def test_controller_hand_made_traces(rk45_ctl):
    """err == 0 grows the step tenfold; err == 1.0 is REJECTED (scipy accepts on err < 1) and shrinks by 0.9; a step that keeps failing
    -- here on NaN norms, what a NaN input gives -- ends below ten spacings of t after a few dozen attempts instead of looping."""
    out = run(rk45_ctl, 1.0, EPS, 1.0, 1.0, 1.0, 0.0, 0.5)
    first = float(out[1]["h_abs"])
    assert first == min(100 * 0.01, 0.01 ** 0.2, 1.0 - EPS)
    h1 = (1.0 - first) - 1.0    # scipy recomputes the step from the rounded t_new
    assert out[2]["accept"] == "1" and float(out[2]["h"]) == h1 and float(out[2]["h_abs"]) == abs(h1) * 10.0
    assert out[3]["accept"] == "1" and float(out[3]["t_new"]) == EPS and out[-1]["kind"] == "done" and out[-1]["attempts"] == "2"
    out = run(rk45_ctl, 1.0, EPS, 1.0, 1.0, 1.0, 1.0, 0.5, 0.5)
    assert out[2]["accept"] == "0" and float(out[2]["h_abs"]) == abs(h1) * 0.9 and float(out[2]["t_new"]) == 1.0 - first
    # the retry starts from the same t with the shrunk step; accepted after a rejection, the factor min(10, 0.9 * 0.5^-0.2) > 1 is capped at 1
    h2 = (1.0 - abs(h1) * 0.9) - 1.0
    assert 0.9 * 0.5 ** -0.2 > 1
    assert out[3]["accept"] == "1" and float(out[3]["t"]) == 1.0 and float(out[3]["h"]) == h2 and float(out[3]["h_abs"]) == abs(h2)
    for bad in (float("nan"), 1e300):
        out = run(rk45_ctl, 1.0, EPS, 1.0, 1.0, 1.0, *[bad] * 64)
        assert out[-1]["kind"] == "small" and 10 < int(out[-1]["attempts"]) < 40 and float(out[-1]["t"]) == 1.0
        assert float(out[-1]["h_abs"]) < float(out[-1]["min_step"]) == 10 * np.spacing(1.0) / 2
        assert all(a["accept"] == "0" for a in out[2:-1])


def test_argument_errors_come_before_any_device():
    import torch
    import flowdec_amd
    s = flowdec_amd.from_preset("baseline_scoredec_75s", nf=8)
    y = torch.zeros(1, 1, 12000)
    with pytest.raises(ValueError, match="driver"):
        s.enhance(y, sampler_type="ode", driver="bogus")
    with pytest.raises(ValueError, match="RK45"):
        s.enhance(y, sampler_type="ode", driver="device", method="RK23")
    with pytest.raises(ValueError, match="max_step"):
        s.enhance(y, sampler_type="ode", driver="device", max_step=0.1)
    with pytest.raises(ValueError, match="atol"):
        s.enhance(y, sampler_type="ode", driver="device", atol=0.0)
    clips = [torch.zeros(12000), torch.zeros(12500)]
    with pytest.raises(ValueError, match="atol"):
        s.enhance_ode_batch(clips, atol=0)
    with pytest.raises(ValueError, match="rtol"):
        s.enhance_ode_batch(clips, rtol=-1e-3)
    with pytest.raises(ValueError, match="only one"):
        s.enhance_ode_batch(clips, seeds=[1, 2], generator=torch.Generator())
    with pytest.raises(ValueError, match="ode"):           # as before: the batch entry point of the PC sampler does not take it
        s.enhance_batch(clips, sampler_type="ode")
    with pytest.raises(RuntimeError, match="GPU"):         # no CPU compute path
        s.enhance_ode_batch(clips)
    with pytest.raises(RuntimeError, match="GPU"):
        s.enhance(y, sampler_type="ode", driver="device")


def test_abi_is_bound_and_refuses_without_a_model():
    import ctypes as C
    from flowdec_amd import _lib as L
    lib = L.load()
    for name in ("fd_score_ode_workspace_bytes", "fd_score_ode_solve", "fd_score_ode_enhance_workspace_bytes", "fd_score_ode_enhance",
                 "fd_score_update_clips"):
        assert getattr(lib, name).argtypes == L.SIGNATURES[name][1]
    assert L.STEP_CONTROL == dict(batch=0, clip=1)
    assert lib.fd_score_ode_workspace_bytes(None, 1, 64, 0) == 0 and lib.fd_score_ode_enhance_workspace_bytes(None, 1, 12000, 1) == 0
    cfg = L.FdScoreConfig(THETA, SIGMA_MIN, SIGMA_MAX, EPS, 0.0, 30, 0, 1, 0, 1)
    assert lib.fd_score_ode_solve(None, None, None, None, C.byref(cfg), 1e-3, 1e-3, 0, None, None, None, None, 1, 64, None, 0, None) != 0
    assert b"null model" in lib.fd_last_error()
    # the operator-level entry refuses before any launch, with a message that names it
    assert lib.fd_score_update_clips(None, None, None, None, None, None, 1, 8, 8, 1, L.FD_F32, None) != 0
    assert b"fd_score_update_clips" in lib.fd_last_error()


def test_parser_and_keyword_builder():
    import flowdec_amd
    from flowdec_amd.enhance_cli import batchable, build_parser, enhance_kwargs, ode_sampler
    p = build_parser()
    a = p.parse_args(BASE)
    assert (a.sampler, a.ode_rtol, a.ode_atol) == ("pc", 1e-5, 1e-5)
    assert p.parse_args(BASE + ["--sampler", "ode"]).sampler == "ode"
    with pytest.raises(SystemExit):
        p.parse_args(BASE + ["--sampler", "bogus"])
    score = flowdec_amd.from_preset("baseline_scoredec_75s", nf=8)
    flow = flowdec_amd.from_preset("flowdec_75m", nf=8)
    # without --sampler (and with --sampler pc) the dict is today's, exactly
    for args in (a, p.parse_args(BASE + ["--sampler", "pc"])):
        assert enhance_kwargs(score, args) == dict(N=2, predictor="reverse_diffusion", corrector="ald", snr=0.5) and not ode_sampler(score, args)
    ode = p.parse_args(BASE + ["--sampler", "ode", "--ode-rtol", "1e-3", "--ode-atol", "1e-2", "--predictor", "euler_maruyama"])
    assert ode_sampler(score, ode) and batchable(score, ode)
    assert enhance_kwargs(score, ode) == dict(N=2, rtol=1e-3, atol=1e-2)
    assert not ode_sampler(flow, ode) and enhance_kwargs(flow, ode) == dict(N=2, solver="midpoint")
