"""The ScoreDec ODE sampler on the device (fd_score_ode_solve / fd_score_ode_enhance; ScoreModel.enhance(sampler_type='ode', driver='device'),
ScoreModel.enhance_ode_batch, enhance_cli --sampler ode) on the nf-8 baseline of tests/test_hip_baselines.py: the per-clip score epilogue
bit for bit against the scalar kernel, the reference's own golden, the host driver, batch invariance under per-clip step control, the noise
sources, the refusals, and the command line."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import solver_ops_ref as R
from conftest import load_golden, rel_err
from oracle import flowdec_oracle as O
from test_hip_baselines import baseline
from test_hip_ops import check

pytestmark = pytest.mark.gpu
DT = {"bf16": torch.bfloat16, "fp32": torch.float32}
TOL_WAVE = 2e-3      # what test_score_ode_sampler_golden grants the host driver against the reference's golden
TOL_EVAL = 1e-5      # what it grants fd_score_eval against the float64 statement of the drift
_host = {}


def ode(m, y, driver, tol, **kw):
    return m.enhance(y, sampler_type="ode", driver=driver, N=30, rtol=tol, atol=tol, return_nfe=True, **kw)


def golden_case():
    g = load_golden("g13_score_nf8.npz")
    Tp = O.padded_frames(O.num_frames(g["y"].shape[-1]))
    z0 = torch.from_numpy(next(O.seeded_noises(int(g["noise_seed"]), (1, 1, 768, Tp))))   # the fixture's single-clip stream
    return g, torch.from_numpy(g["y"][:1]), z0


def host_result(tol):
    """The host driver on the golden's first clip and noise, computed once per tolerance."""
    if tol not in _host:
        _, y, z0 = golden_case()
        _host[tol] = ode(baseline("score", "fp32"), y, "host", tol, noise=z0)
    return _host[tol]


def three_clips():
    """Noise, a tone and a click, of different lengths in one T_pad = 64 bucket (normalize='noisy' removes the level, not the content)."""
    rng = np.random.default_rng(7)
    n = np.arange(12500)
    noise = 0.1 * rng.standard_normal(12000)
    tone = 0.3 * np.sin(2 * np.pi * 440.0 / 48000.0 * n[:11000])
    click = 0.001 * rng.standard_normal(12500)
    click[6000:6010] = 0.5
    return [torch.from_numpy(c.astype(np.float32)) for c in (noise, tone, click)]


# ---- 4. the per-clip epilogue ---------------------------------------------------------------------------------------------------------------
def coefficients(t, denoise, N=30, theta=1.5, smin=0.05, smax=0.5):
    """(cb, cy, cn) of fd_score_eval at time t in float64: the drift theta (y - x) - g^2 / 2 score with score = -v / std, or the mean of the
    noise-free reverse-diffusion step of dt = 1 / N."""
    ls = np.log(smax / smin)
    std = np.sqrt(smin ** 2 * np.exp(-2 * theta * t) * (np.exp(2 * (theta + ls) * t) - 1) * ls / (theta + ls))
    g2 = (smin * (smax / smin) ** t) ** 2 * 2 * ls
    if denoise:
        return 1 + theta / N, -theta / N, -(g2 / N) / std
    return -theta, theta, 0.5 * g2 / std


@pytest.mark.parametrize("ks", [1, 3])
@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_epilogue_per_clip_equals_scalar_kernel(dtype, ks):
    """fd_score_update_clips on B = 3 clips at the times (1.0, 0.4, 0.03): every clip is the scalar-coefficient kernel on that clip alone,
    bit for bit, in drift and in denoise mode, on the model's 768 x 64 plane and on a small odd image; and both agree with the float64
    statement cb x + cy y + cn v within the bound the suite uses for fd_score_eval.  A clip whose cy is 0 does not read Y."""
    from flowdec_amd import ops
    plane = lambda a: torch.view_as_complex(torch.from_numpy(np.ascontiguousarray(a, np.float32))).cuda()
    rng = np.random.default_rng(40 + ks)
    for shape in ((3, 768, 64), (3, 24, 20)):
        w = R.output_weights(rng, ks, False)
        pyr, (base, Y, _, _) = R.image_data(rng, shape, dtype, False)
        dpyr, dw, dbase, dY = torch.from_numpy(pyr).cuda().to(DT[dtype]), torch.from_numpy(w).cuda(), plane(base), plane(Y)
        for denoise in (False, True):
            tab = np.array([coefficients(t, denoise) for t in (1.0, 0.4, 0.03)], np.float32)
            got = ops.score_update_clips(dpyr, dw, dbase, dY, torch.from_numpy(tab).cuda(), dst=plane(R.sentinel(shape + (2,))))
            for b in range(3):
                cb, cy, cn = (float(v) for v in tab[b])
                one = ops.score_update(dpyr[b:b + 1].contiguous(), dw, dbase[b:b + 1].contiguous(), cb, dY[b:b + 1].contiguous(), cy, cn, 0.0)
                assert torch.equal(torch.view_as_real(got[b:b + 1]), torch.view_as_real(one)), (shape, denoise, b)
                ref = R.score_update_ref(pyr[b:b + 1], w, base[b:b + 1], cb, Y[b:b + 1], cy, cn, None, 0.0)
                err = rel_err(torch.view_as_real(got[b:b + 1]).cpu().numpy(), ref)
                print(f"epilogue[{dtype} ks={ks} {shape} denoise={denoise} clip {b}]: rel_err {err:.2e}")
                assert err < TOL_EVAL
        # cy == 0 for clip 1 only: its Y (NaNs) is never read, the other clips read theirs
        tab = np.array([coefficients(t, False) for t in (1.0, 0.4, 0.03)], np.float32)
        tab[1, 1] = 0.0
        Yn = Y.copy()
        Yn[1] = np.nan
        got = torch.view_as_real(ops.score_update_clips(dpyr, dw, dbase, plane(Yn), torch.from_numpy(tab).cuda())).cpu().numpy()
        assert np.isfinite(got).all()
        for b in range(3):
            cb, cy, cn = (float(v) for v in tab[b])
            assert rel_err(got[b:b + 1], R.score_update_ref(pyr[b:b + 1], w, base[b:b + 1], cb, Y[b:b + 1], cy, cn, None, 0.0)) < TOL_EVAL


# ---- 5. / 6. the reference's golden and the host driver -------------------------------------------------------------------------------------
def test_device_driver_reference_golden():
    """The device driver against the reference's own ODE sampler (scipy RK45 at rtol = atol = 1e-3): scipy's NFE, and the waveform within
    the tolerance the host driver is granted against the same golden."""
    g, y, z0 = golden_case()
    out, nfe = ode(baseline("score", "fp32"), y, "device", 1e-3, noise=z0)
    print(f"device driver: nfe {nfe} (golden {int(g['ode_rk45_nfe'])})")
    assert out.shape == g["ode_rk45"].shape and out.device.type == "cpu"
    assert nfe == int(g["ode_rk45_nfe"])
    check("score_ode_device_vs_golden[fp32]", out.numpy(), g["ode_rk45"], TOL_WAVE)


@pytest.mark.parametrize("tol", [1e-3, 1e-2])
def test_device_driver_equals_host_driver(tol):
    m = baseline("score", "fp32")
    _, y, z0 = golden_case()
    host, nfe_host = host_result(tol)
    dev, nfe_dev = ode(m, y, "device", tol, noise=z0)
    print(f"tol {tol}: nfe host {nfe_host} device {nfe_dev}")
    if tol == 1e-3:
        assert nfe_dev == nfe_host
    check(f"score_ode_device_vs_host[fp32, tol={tol}]", dev.numpy(), host.numpy(), TOL_WAVE)


def test_device_driver_batch_global_equals_host_driver():
    """B = 2 clips of one length through enhance(): ONE controller on the norms of the whole batch, as solve_ivp sees the flattened state."""
    g = load_golden("g13_score_nf8.npz")
    m = baseline("score", "fp32")
    y = torch.from_numpy(g["y"])
    Tp = O.padded_frames(O.num_frames(y.shape[-1]))
    z = torch.from_numpy(next(O.seeded_noises(int(g["noise_seed"]) + 1, (2, 1, 768, Tp))))
    host, nfe_host = ode(m, y, "host", 1e-3, noise=z)
    dev, nfe_dev = ode(m, y, "device", 1e-3, noise=z)
    print(f"B = 2: nfe host {nfe_host} device {nfe_dev}")
    assert dev.shape == host.shape == y.shape
    check("score_ode_device_vs_host[fp32, B=2]", dev.numpy(), host.numpy(), TOL_WAVE)
    # other options of enhance()
    x, info = m.enhance(y, sampler_type="ode", driver="device", N=30, rtol=1e-3, atol=1e-3, noise=z, return_preprocess_info=True)
    assert torch.equal(x, dev) and info["orig_length"] == y.shape[-1] and tuple(info["normfac"].shape) == (2, 1, 1)
    nod, _ = ode(m, y, "device", 1e-3, noise=z, denoise=False)
    assert not torch.equal(nod, dev) and torch.isfinite(nod).all()


# ---- 7. / 8. per-clip step control ----------------------------------------------------------------------------------------------------------
def test_batch_invariance_under_per_clip_control():
    """Three clips of different lengths and content in one bucket: every output of enhance_ode_batch is the one-clip device call, bit for
    bit, with its NFE, in any order; the NFE differ, so a finished clip really rides along."""
    m = baseline("score", "fp32")
    clips, seeds = three_clips(), [31, 32, 33]
    singles = [ode(m, c, "device", 1e-2, seed=[s]) for c, s in zip(clips, seeds)]
    for order in ((0, 1, 2), (2, 0, 1)):
        outs, nfe = m.enhance_ode_batch([clips[i] for i in order], N=30, rtol=1e-2, atol=1e-2, seeds=[seeds[i] for i in order], return_nfe=True)
        print(f"order {order}: nfe {nfe}, evals {m.last_evals}, rejected {m.last_rejected_per_clip.tolist()}")
        for k, i in enumerate(order):
            assert outs[k].shape == clips[i].shape and torch.equal(outs[k], singles[i][0]), (order, i)
            assert nfe[k] == singles[i][1], (order, i)
        assert m.last_evals == max(nfe) and m.last_nfe_per_clip.tolist() == nfe
    assert len(set(s[1] for s in singles)) > 1, "the three clips take the same number of attempts: no clip rides along"


def test_noise_sources():
    """seed= is the explicit plane fd_noise_fill writes for the seed, bit for bit, on both entry points; generator= draws, clip by clip,
    what the one-clip calls draw."""
    from flowdec_amd.noise import noise_fill, seeds_to_tensor
    m = baseline("score", "fp32")
    clips, seeds = three_clips()[:2], [31, 32]
    F, _, Tp = m._frames(12000)
    planes = [noise_fill(seeds_to_tensor([s], 1, "cuda"), F, Tp)[0] for s in seeds]
    kw = dict(N=30, rtol=1e-2, atol=1e-2)
    seeded = m.enhance_ode_batch(clips, seeds=seeds, **kw)
    explicit = m.enhance_ode_batch(clips, noise=planes, **kw)
    assert all(torch.equal(a, b) for a, b in zip(seeded, explicit))
    one = m.enhance(clips[1], sampler_type="ode", driver="device", noise=planes[1], **kw)
    assert torch.equal(one, seeded[1]) and torch.equal(one, m.enhance(clips[1], sampler_type="ode", driver="device", seed=[32], **kw))
    drawn = m.enhance_ode_batch(clips, generator=torch.Generator(device="cuda").manual_seed(5), **kw)
    gen = torch.Generator(device="cuda").manual_seed(5)
    for c, d in zip(clips, drawn):
        assert torch.equal(d, m.enhance(c, sampler_type="ode", driver="device", generator=gen, **kw))
    assert not torch.equal(drawn[0], seeded[0])


# ---- 9. refusals ----------------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing():
    from flowdec_amd import _lib as L
    m = baseline("score", "fp32")
    lib, h = L.load(), m.backbone.handle()
    p, N = C.c_void_p(8), None
    cfg = L.FdScoreConfig(1.5, 0.05, 0.5, 0.03, 0.0, 30, 0, 1, 0, 1)
    nfe = (C.c_int * 300)()
    solve = lambda cfg=cfg, rtol=1e-3, atol=1e-3, ctl=1, B=1, ws=1 << 40, noise=p, seeds=N: lib.fd_score_ode_solve(
        h, p, noise, seeds, C.byref(cfg), rtol, atol, ctl, p, nfe, N, N, B, 64, p, ws, N)
    wave = lambda ctl=1, B=1, ws=1 << 40, atol=1e-3: lib.fd_score_ode_enhance(h, p, N, p, N, C.byref(cfg), 1e-3, atol, ctl, p, nfe, N, N, B, 12000, p, ws, N)
    bad = L.FdScoreConfig(1.5, 0.5, 0.05, 0.03, 0.0, 30, 0, 1, 0, 1)    # sigma_max < sigma_min
    for label, call, rc, msg in (
            ("too many clips", lambda: solve(B=257), -1, "at most 256 clips"),
            ("too many clips (waveform)", lambda: wave(B=257), -1, "at most 256 clips"),
            ("short workspace", lambda: solve(ws=1024), -3, "workspace 1024 < required"),
            ("short workspace (waveform)", lambda: wave(ws=1024), -3, "workspace 1024 < required"),
            ("short workspace (batch)", lambda: solve(ctl=0, B=2, ws=1024), -3, "workspace 1024 < required"),
            ("OUVE", lambda: solve(cfg=bad), -1, "OUVE"),
            ("atol", lambda: solve(atol=0.0), -1, "atol > 0"),
            ("atol (waveform)", lambda: wave(atol=0.0), -1, "atol > 0"),
            ("rtol", lambda: solve(rtol=-1.0), -1, "rtol >= 0"),
            ("both noise sources", lambda: solve(seeds=p), -1, "exactly one"),
            ("no noise source", lambda: solve(noise=N), -1, "exactly one"),
            ("step control", lambda: solve(ctl=2), -1, "step_control")):
        assert call() == rc, label
        assert msg in lib.fd_last_error().decode(), (label, lib.fd_last_error())
    assert lib.fd_score_ode_workspace_bytes(h, 257, 64, 1) == 0 and lib.fd_score_ode_workspace_bytes(h, 257, 64, 0) > 0
    assert lib.fd_score_ode_enhance_workspace_bytes(h, 3, 12000, 1) > lib.fd_enhance_workspace_bytes(h, 3, 12000)
    assert not any(nfe)


def test_nan_input_is_an_error_not_a_hang():
    """A NaN sample makes every error norm NaN: each attempt is rejected and shrinks the step by 0.2 until it falls below ten spacings of t
    (tests/test_score_ode_cpu.py drives that arithmetic on the host), and the library's message surfaces as an exception."""
    m = baseline("score", "fp32")
    y = three_clips()[0].clone()
    y[5000] = float("nan")
    with pytest.raises(RuntimeError, match="step size too small|step limit reached"):
        m.enhance(y, sampler_type="ode", driver="device", N=30, rtol=1e-2, atol=1e-2, seed=[1])
    out = m.enhance(three_clips()[0], sampler_type="ode", driver="device", N=30, rtol=1e-2, atol=1e-2, seed=[1])   # the model is usable afterwards
    assert torch.isfinite(out).all()


# ---- 10. the command line -------------------------------------------------------------------------------------------------------------------
def test_cli_sampler_ode_and_pc(tmp_path, capsys):
    """--sampler ode writes, byte for byte, what enhance_ode_batch gives on the same clips and seeds, prints one NFE per file and says that
    the predictor-corrector options are ignored; --sampler pc (and no --sampler) writes what enhance_batch gives, as before."""
    from flowdec_amd import enhance_cli
    from flowdec_amd.noise import clip_seed
    m = baseline("score", "fp32")
    os.makedirs(tmp_path / "in")
    for name, c in zip("abc", three_clips()):
        enhance_cli.save_wav(str(tmp_path / "in" / f"{name}.wav"), c[None], 48000)
    clips = [enhance_cli.load_wav(str(tmp_path / "in" / f"{name}.wav"))[0] for name in "abc"]
    seeds = [clip_seed(7, i) for i in range(3)]
    common = ["--ckpt", "unused.ckpt", "--files", str(tmp_path / "in"), "--N", "3", "--precision", "fp32", "--rng", "native", "--seed", "7"]

    def same_files(outdir, waves):
        os.makedirs(tmp_path / "want", exist_ok=True)
        for name, w in zip("abc", waves):
            enhance_cli.save_wav(str(tmp_path / "want" / f"{name}.wav"), w.cpu(), 48000)
            assert open(tmp_path / outdir / f"{name}.wav", "rb").read() == open(tmp_path / "want" / f"{name}.wav", "rb").read(), (outdir, name)

    res = enhance_cli.run(common + ["--outdir", str(tmp_path / "ode"), "--sampler", "ode", "--ode-rtol", "1e-2", "--ode-atol", "1e-2"], model=m)
    printed = capsys.readouterr().out
    assert res.n_done == 3 and printed.count("NFE ") == 3 and printed.count("are ignored") == 1
    want, nfe = m.enhance_ode_batch(clips, N=3, rtol=1e-2, atol=1e-2, seeds=seeds, return_nfe=True)
    same_files("ode", want)
    assert all(f"NFE {n}: " in printed for n in nfe)
    # one file per call is the same per-file controller
    res = enhance_cli.run(common + ["--outdir", str(tmp_path / "ode1"), "--sampler", "ode", "--ode-rtol", "1e-2", "--ode-atol", "1e-2", "--batch-files", "1"], model=m)
    assert res.n_done == 3 and capsys.readouterr().out.count("are ignored") == 1
    same_files("ode1", want)
    pc = m.enhance_batch(clips, N=3, predictor="reverse_diffusion", corrector="ald", snr=0.5, seeds=seeds)
    for outdir, extra in (("pc", ["--sampler", "pc"]), ("default", [])):
        assert enhance_cli.run(common + ["--outdir", str(tmp_path / outdir)] + extra, model=m).n_done == 3
        same_files(outdir, pc)
    assert "are ignored" not in capsys.readouterr().out
