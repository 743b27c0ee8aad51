"""Per-clip step control of the adaptive solvers ('dopri5', 'tsit5'): FlowModel.enhance / enhance_batch(step_control='clip'),
fd_ode_solve_adaptive_clips, the CLI's --step-control clip.

The batch-global controller (torchdyn's behaviour for a batched call) accepts or rejects a step on ONE error ratio over the whole batch,
so a clip's waveform depends on its companions.  With step_control='clip' every clip has its own t, dt, checkpoint index and decisions,
and the contract is the one of every other batched path here: clip b is BIT-IDENTICAL, waveform and realised NFE, to the one-clip call
`m.enhance(clip, solver=..., noise=... / seed=..., atol=, rtol=)` -- the path a user of the reference's file-by-file driver gets
(enhance.py:96-137), which this feature leaves untouched.  Every comparison is torch.equal: there is no tolerance."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import flowdec_oracle as O
from test_cli import synthetic_ckpt

pytestmark = pytest.mark.gpu

F, TP, N, TOL = 768, 64, 2, 1e-2
# one T_pad = 64 bucket (L <= 24575), different lengths
LENS = [12000, 20000, 15000, 17001]
SOLVERS = ("dopri5", "tsit5")
_models, _refs = {}, {}


def model(precision):
    if precision not in _models:
        import flowdec_amd
        m = flowdec_amd.from_preset("flowdec_75m", precision=precision, nf=8)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in O.random_state_dict(seed=8, nf=8).items()}, strict=False)
        _models[precision] = m.cuda()
    return _models[precision]


def clips():
    """Four clips of different character, so that their solves differ: white noise, a tone in weak noise, a decaying click train, noise
    that fades in (the front end normalises every clip by its own maximum, so the level alone would change nothing)."""
    rng = np.random.default_rng(0)
    t = [np.arange(n) / 48000.0 for n in LENS]
    c = [0.1 * rng.standard_normal(LENS[0]),
         0.5 * np.sin(2 * np.pi * 440.0 * t[1]) + 0.002 * rng.standard_normal(LENS[1]),
         np.where(np.arange(LENS[2]) % 2400 == 0, 1.0, 0.0) * np.exp(-3.0 * t[2] * 48000.0 / LENS[2]) + 0.001 * rng.standard_normal(LENS[2]),
         0.3 * np.linspace(0.0, 1.0, LENS[3]) ** 2 * rng.standard_normal(LENS[3])]
    return [torch.from_numpy(v.astype(np.float32)) for v in c]


def noises(seed=100):
    g = torch.Generator().manual_seed(seed)
    return [torch.view_as_complex(torch.randn(1, 1, F, TP, 2, generator=g) / np.sqrt(2)) for _ in LENS]


def one_by_one(precision, solver):
    """The yardstick, computed once per (precision, solver): the one-clip calls WITHOUT the new keyword -> [(waveform, nfe)]."""
    key = (precision, solver)
    if key not in _refs:
        m = model(precision)
        out = []
        for c, z in zip(clips(), noises()):
            w = m.enhance(c, N=N, solver=solver, noise=z, atol=TOL, rtol=TOL)
            assert torch.isfinite(w).all() and w.abs().max() > 0
            out.append((w, m.last_nfe))
        _refs[key] = out
    return _refs[key]


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_per_sample_time_equals_the_scalar_time_call(precision):
    """The network with a device array of per-sample times: row b gets the arithmetic of the scalar-t call on clip b alone (time
    embedding, Dense_0 biases, every convolution's bias row).  The per-clip controller rests on this."""
    m = model(precision)
    g = torch.Generator().manual_seed(1)
    x = torch.view_as_complex(torch.randn(3, 1, F, TP, 2, generator=g)).cuda()
    y = torch.view_as_complex(torch.randn(3, 1, F, TP, 2, generator=g)).cuda()
    t = torch.tensor([0.03, 0.5, 0.97], device="cuda")
    v = m(x, y, t)
    assert torch.isfinite(torch.view_as_real(v)).all()
    for b in range(3):
        vb = m(x[b:b + 1], y[b:b + 1], t[b:b + 1])
        assert torch.equal(torch.view_as_real(vb), torch.view_as_real(v[b:b + 1])), f"clip {b}: per-sample t differs from the scalar-t call"
    assert not torch.equal(torch.view_as_real(m(x[:1], y[:1], t[1:2])), torch.view_as_real(v[:1]))   # the time does matter


@pytest.mark.parametrize("precision", ["bf16x3", "fp32"])
@pytest.mark.parametrize("solver", SOLVERS)
def test_batch_equals_one_by_one(solver, precision):
    ref = one_by_one(precision, solver)
    m = model(precision)
    outs = m.enhance_batch(clips(), N=N, solver=solver, step_control="clip", noise=noises(), atol=TOL, rtol=TOL)
    nfe, rej, evals = m.last_nfe_per_clip.tolist(), m.last_rejected_per_clip, m.last_evals
    print(f"{solver}[{precision}]: one-by-one nfe {[n for _, n in ref]}, batch nfe {nfe}, rejected {rej.tolist()}, batch evaluations {evals}")
    # the inputs exercise the per-clip logic: clips that need different numbers of steps, and at least one rejected attempt
    assert len({n for _, n in ref}) >= 2, "the one-by-one runs all realise the same NFE: choose other clips"
    assert rej.sum() > 0, "no clip rejects a step: choose other clips"
    for b, (w, n) in enumerate(ref):
        assert outs[b].shape == w.shape
        assert torch.equal(outs[b], w), f"clip {b}: batch with per-clip control != the one-clip call"
        assert nfe[b] == n, f"clip {b}: NFE {nfe[b]} != {n} of the one-clip call"
    # the counters: every attempt is six evaluations after the two of the initial step; the batch runs as long as its slowest clip
    assert m.last_nfe == max(nfe) == evals
    assert all((n - 2) % 6 == 0 and (n - 2) // 6 - int(r) >= N for n, r in zip(nfe, rej))


@pytest.mark.parametrize("solver", SOLVERS)
def test_shard_invariance(solver):
    """clips[:k] and clips[k:] as two calls = the whole batch, clip for clip (what sharded_enhance needs of an adaptive solver)."""
    ref = one_by_one("bf16x3", solver)
    m = model("bf16x3")
    cl, nz = clips(), noises()
    for k in (1, 3):
        got = m.enhance_batch(cl[:k], N=N, solver=solver, step_control="clip", noise=nz[:k], atol=TOL, rtol=TOL)
        nfe = m.last_nfe_per_clip.tolist()
        got += m.enhance_batch(cl[k:], N=N, solver=solver, step_control="clip", noise=nz[k:], atol=TOL, rtol=TOL)
        nfe += m.last_nfe_per_clip.tolist()
        for b, (w, n) in enumerate(ref):
            assert torch.equal(got[b], w) and nfe[b] == n, f"split at {k}: clip {b} differs from the one-clip call"


def equal_length_batch():
    """The four clips cut to one length: a [B, 1, L] batch for `enhance`."""
    Lw = min(LENS)
    return torch.stack([c[:Lw] for c in clips()])[:, None], torch.cat(noises())


def test_equal_lengths_and_the_default_is_unchanged():
    m = model("bf16x3")
    y, nz = equal_length_batch()
    kw = dict(N=N, solver="dopri5", atol=TOL, rtol=TOL)
    got = m.enhance(y, step_control="clip", noise=nz, **kw)
    nfe = m.last_nfe_per_clip.tolist()
    single = []
    for b in range(len(LENS)):
        w = m.enhance(y[b:b + 1], noise=nz[b:b + 1], **kw)
        assert torch.equal(got[b:b + 1], w) and nfe[b] == m.last_nfe, f"clip {b}: enhance(step_control='clip') != the one-clip call"
        single.append(w)
        # one clip: both controllers are the same thing
        assert torch.equal(m.enhance(y[b:b + 1], noise=nz[b:b + 1], step_control="clip", **kw), w) and m.last_nfe == nfe[b]
    # step_control=None / 'batch' = the call without the keyword: the batch-global controller, which is NOT the per-clip result
    plain = m.enhance(y, noise=nz, **kw)
    n_plain = m.last_nfe
    for sc in (None, "batch"):
        assert torch.equal(m.enhance(y, noise=nz, step_control=sc, **kw), plain) and m.last_nfe == n_plain
    assert not torch.equal(plain, got), "the batch-global controller gave the per-clip result: the batch does not exercise the difference"
    with pytest.raises(ValueError, match="step_control"):
        m.enhance(y, N=N, solver="midpoint", step_control="clip", noise=nz)


@pytest.mark.parametrize("source", ["noise", "seed"])
@pytest.mark.parametrize("solver", SOLVERS)
def test_one_clip_batch_control_equals_clip_control(solver, source):
    """ONE clip: step_control='batch' and 'clip' are the same solve, waveform and NFE, from a noise plane and from a seed.  The two modes
    share their host loop (solve.hip: adaptive_solve) and differ in a policy; this case keeps the two policies one algorithm."""
    from flowdec_amd.noise import clip_seed
    m = model("bf16x3")
    src = dict(noise=noises()[0]) if source == "noise" else dict(seed=[clip_seed(21, 0)])
    kw = dict(N=N, solver=solver, atol=TOL, rtol=TOL, **src)
    c = clips()[0]                                                   # 12000 samples
    a = m.enhance(c, step_control="batch", **kw)
    n_a = m.last_nfe
    b = m.enhance(c, step_control="clip", **kw)
    assert torch.isfinite(a).all() and a.abs().max() > 0
    assert torch.equal(a, b), "one clip: the batch-global controller != the per-clip controller"
    assert n_a == m.last_nfe == int(m.last_nfe_per_clip[0]) == m.last_evals and (n_a - 2) % 6 == 0 and (n_a - 2) // 6 >= N


@pytest.mark.parametrize("solver", SOLVERS)
def test_seeded(solver):
    """seeds= draws the initial plane inside the solver: clip b = enhance(clip_b, seed=[s_b]) of today, and = the buffer form on
    noise_fill's planes."""
    from flowdec_amd.noise import clip_seed, noise_fill, seeds_to_tensor
    m = model("bf16x3")
    cl = clips()
    seeds = [clip_seed(21, b) for b in range(len(cl))]
    kw = dict(N=N, solver=solver, atol=TOL, rtol=TOL)
    got = m.enhance_batch(cl, seeds=seeds, step_control="clip", **kw)
    nfe = m.last_nfe_per_clip.tolist()
    planes = noise_fill(seeds_to_tensor(seeds, len(cl), "cuda"), F, TP)[0]      # [B, 1, F, TP]
    buf = m.enhance_batch(cl, noise=[planes[b:b + 1] for b in range(len(cl))], step_control="clip", **kw)
    for b, c in enumerate(cl):
        ref = m.enhance(c, seed=[seeds[b]], **kw)
        assert torch.isfinite(ref).all() and ref.abs().max() > 0
        assert torch.equal(got[b], ref) and nfe[b] == m.last_nfe, f"clip {b}: seeded batch != the seeded one-clip call"
        assert torch.equal(buf[b], ref), f"clip {b}: the buffer form on noise_fill's plane != the seeded form"
    # enhance(seed=, step_control='clip') on an equal-length batch goes straight to the seeded form too
    y, _ = equal_length_batch()
    a = m.enhance(y, seed=seeds, step_control="clip", **kw)
    for b in range(len(cl)):
        assert torch.equal(a[b:b + 1], m.enhance(y[b:b + 1], seed=[seeds[b]], **kw))


def test_trajectory():
    m = model("bf16x3")
    y, nz = equal_length_batch()
    kw = dict(N=N, solver="tsit5", atol=TOL, rtol=TOL, return_traj=True)
    traj, waves = m.enhance(y, noise=nz, step_control="clip", **kw)
    assert traj.shape == (N + 1, len(LENS), 1, F, TP) and len(waves) == N + 1
    for b in range(len(LENS)):
        tb, wb = m.enhance(y[b:b + 1], noise=nz[b:b + 1], **kw)
        for i in range(N + 1):
            assert torch.equal(torch.view_as_real(traj[i, b:b + 1]), torch.view_as_real(tb[i])), f"clip {b}, checkpoint {i}: state differs"
            assert torch.equal(waves[i][b:b + 1], wb[i]), f"clip {b}, checkpoint {i}: waveform differs"
        assert torch.view_as_real(tb[1] - tb[0]).abs().max() > 0 and torch.view_as_real(tb[2] - tb[1]).abs().max() > 0


SPEC = [("a", 12000), ("b", 20000), ("c", 30000), ("d", 12000), ("e", 30000), ("f", 20000)]   # two buckets: T_pad 64 (a b d f), 128 (c e)


def test_cli_step_control_clip(tmp_path, monkeypatch):
    """--solver dopri5 --step-control clip --batch-files 4 writes the files of --batch-files 1, bit for bit, with torch generators and with
    the library's seeds; the batched run really runs batches."""
    from flowdec_amd import enhance_cli
    ckpt = synthetic_ckpt()
    for sd in (ckpt["state_dict"], ckpt["_pl_ema_state_dict"]):
        sd["backbone.output_layer.weight"] = sd["backbone.output_layer.weight"] * 0.02
    torch.save(ckpt, tmp_path / "m.ckpt")
    (tmp_path / "in").mkdir()
    rng = np.random.default_rng(2)
    for name, n in SPEC:
        enhance_cli.save_wav(str(tmp_path / "in" / f"{name}.wav"), torch.from_numpy((0.1 * rng.standard_normal((1, n))).astype(np.float32)), 48000)
    common = ["--ckpt", str(tmp_path / "m.ckpt"), "--files", str(tmp_path / "in"), "--N", "2", "--solver", "dopri5", "--step-control", "clip", "--seed", "4",
              "--precision", "bf16x3"]
    model_ = enhance_cli.load_from_checkpoint(str(tmp_path / "m.ckpt"), map_location="cuda:0", precision="bf16x3")
    calls = []
    batch_call = type(model_).enhance_batch

    def counting(self, clips_, **kw):
        calls.append((len(clips_), kw.get("step_control")))
        return batch_call(self, clips_, **kw)

    def run(name, extra):
        res = enhance_cli.run(common + ["--outdir", str(tmp_path / name)] + extra, model=model_)
        assert res.n_done == len(SPEC)
        return {n: (tmp_path / name / f"{n}.wav").read_bytes() for n, _ in SPEC}

    monkeypatch.setattr(type(model_), "enhance_batch", counting)
    one = run("o1", ["--batch-files", "1"])
    n1 = run("n1", ["--batch-files", "1", "--rng", "native"])
    assert not calls
    four = run("o4", ["--batch-files", "4"])
    n4 = run("n4", ["--batch-files", "4", "--rng", "native"])
    assert sorted(calls) == [(2, "clip"), (2, "clip"), (4, "clip"), (4, "clip")], calls
    for name, _ in SPEC:
        assert four[name] == one[name], f"{name}.wav: --batch-files 4 differs from --batch-files 1"
        assert n4[name] == n1[name], f"{name}.wav: --batch-files 4 differs from --batch-files 1 (--rng native)"
        assert n4[name] != four[name]
    # file b is index 1 of the work list: generator seeded 4 + 1; the default tolerances
    y, _ = enhance_cli.load_wav(str(tmp_path / "in" / "b.wav"))
    ref = model_.enhance(y, N=2, solver="dopri5", generator=torch.Generator(device="cuda:0").manual_seed(5))
    got, _ = enhance_cli.load_wav(str(tmp_path / "o4" / "b.wav"))
    assert torch.equal(got, ref) and torch.isfinite(ref).all() and ref.abs().max() > 0


def test_native_refusals():
    """fd_ode_solve_adaptive_clips says no, with a message, to more than 256 clips, to both or neither of noise and seeds and to a
    workspace that is too small -- before it enqueues anything."""
    from flowdec_amd import _lib as L
    lib = L.load()
    m = model("bf16x3")
    h = m._sync_native()
    B = 2
    Y = torch.zeros(B, 1, F, TP, 2, device="cuda")
    X = torch.full_like(Y, float("nan"))
    nz = torch.zeros_like(Y)
    seeds = torch.zeros(B, dtype=torch.int64, device="cuda")
    need = lib.fd_ode_adaptive_clips_workspace_bytes(h, B, TP)
    assert need > lib.fd_ode_adaptive_workspace_bytes(h, B, TP) > 0
    assert lib.fd_ode_adaptive_clips_workspace_bytes(h, 257, TP) == 0 and lib.fd_ode_adaptive_clips_workspace_bytes(h, B, TP + 1) == 0
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    nfe = (C.c_int * 257)()

    def call(noise, sd, nb, ws_bytes):
        return lib.fd_ode_solve_adaptive_clips(h, L.ptr(Y), L.ptr(noise), L.ptr(sd), 1.0, N, 0, TOL, TOL, L.ptr(X), None, nfe, None, None, nb, TP,
                                               L.ptr(ws), ws_bytes, L.stream())

    for args, msg in (((nz, None, 257, need), b"at most 256 clips"), ((nz, seeds, B, need), b"exactly one of noise and seeds"),
                      ((None, None, B, need), b"exactly one of noise and seeds"), ((nz, None, B, need - 1), b"workspace")):
        assert call(*args) != 0
        assert msg in lib.fd_last_error(), lib.fd_last_error()
    torch.cuda.synchronize()
    assert torch.isnan(X).all(), "a refused call wrote its output"
    assert lib.fd_ode_solve_adaptive_clips(h, L.ptr(Y), L.ptr(nz), None, 1.0, N, 7, TOL, TOL, L.ptr(X), None, nfe, None, None, B, TP, L.ptr(ws), need,
                                           L.stream()) != 0 and b"method" in lib.fd_last_error()
    with pytest.raises(ValueError, match="step_control"):        # the Python layer keeps refusing an adaptive solver without the keyword
        m.enhance_batch(clips(), N=N, solver="tsit5")
