"""Seeded sampler noise on the GPU (include/flowdec_hip.h, "Seeded noise"): the generator against its NumPy restatement
(tests/noise_oracle.py), its distribution, and the bit-identities the seeded entry points promise -- seeded == the buffer call on
fd_noise_fill's output; a clip alone == in a batch == in a ragged bucket == in a shard; graph replay with new seeds."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

import noise_oracle as NO
from conftest import ROOT, load_golden
from oracle import flowdec_oracle as O

pytestmark = pytest.mark.gpu

F = 768
SEEDS = (1000, 1001)
# test_gaussians_match_float64_oracle: the largest error of a component on the 4 x 768 x 256 samples below, measured on an MI355X
# (ROCm 7.2 logf / sqrtf / sincospif): 4.0505e-07.  The kernel and its inputs are deterministic, so the test allows twice that (room
# for another libm or compiler), and never more than 1e-5 (|z| <= 4.08 and a few ulp: anything above is a formula error, not rounding)
MEASURED_MAX_ABS_ERR = 4.0505e-07
_cache = {}


def _seed_tensor(vals):
    from flowdec_amd.noise import seeds_to_tensor
    return seeds_to_tensor(list(vals), len(vals), "cuda")


def _fill(vals, F_, T, draw0=0, n_draws=1, bits=False):
    from flowdec_amd.noise import noise_fill
    return noise_fill(_seed_tensor(vals), F_, T, draw0, n_draws, bits=bits)


def _flow(nf, precision):
    key = ("flow", nf, precision)
    if key not in _cache:
        import flowdec_amd
        m = flowdec_amd.from_preset("flowdec_75m", precision=precision, nf=nf)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in O.random_state_dict(seed=8, nf=nf).items()}, strict=False)
        _cache[key] = m.cuda()
    return _cache[key]


def _wave(B, L, seed=0):
    return torch.from_numpy((0.1 * np.random.default_rng(seed).standard_normal((B, 1, L))).astype(np.float32)).cuda()


def _frames(m, L):
    from flowdec_amd import _lib
    cfg = m.feature_extractor._cfg()
    lib = _lib.load()
    return cfg["n_fft"] // 2 + 1, lib.fd_padded_frames(lib.fd_num_frames(L, cfg["hop"]))


# ---- 1. bits ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F_,T,draw0,n_draws", [(768, 256, 0, 2), (5, 64, 7, 1), (5, 63, 7, 2)])
def test_bits_equal_oracle(F_, T, draw0, n_draws):
    got = _fill(SEEDS, F_, T, draw0, n_draws, bits=True).cpu().numpy()
    assert got.shape == (n_draws, 2, 1, F_, T, 2)
    for d in range(n_draws):
        for b, s in enumerate(SEEDS):
            ra, rb = NO.noise_bits(s, draw0 + d, F_, T)
            assert np.array_equal(got[d, b, 0, :, :, 0], ra.astype(np.int64)), (s, d, "ra")
            assert np.array_equal(got[d, b, 0, :, :, 1], rb.astype(np.int64)), (s, d, "rb")


# ---- 2. Gaussians against float64 on the same uniforms ------------------------------------------------------------------
def test_gaussians_match_float64_oracle():
    z = _fill(SEEDS, F, 256, 0, 2).cpu().numpy()
    worst = 0.0
    for d in range(2):
        for b, s in enumerate(SEEDS):
            ref = NO.noise_plane(s, d, F, 256)
            got = z[d, b, 0].astype(np.complex128)
            worst = max(worst, float(np.abs(got.real - ref.real).max()), float(np.abs(got.imag - ref.imag).max()))
    print(f"seeded noise: max abs error of a component vs float64 = {worst:.4e} (measured {MEASURED_MAX_ABS_ERR:.4e})")
    assert worst < 1e-5, f"{worst:.3e}: a formula error, not rounding"
    assert worst <= 2 * MEASURED_MAX_ABS_ERR, f"{worst:.3e} > 2 x the measured {MEASURED_MAX_ABS_ERR:.3e}"


# ---- 3. distribution ---------------------------------------------------------------------------------------------------
def test_distribution():
    """Per plane (n = 768 x 256 complex samples; components scaled to unit variance), each statistic in units of its own standard
    error stays within 4: means (1/sqrt n), variances - 1 (sqrt 2 / sqrt n), re.im covariance (1/sqrt n), lag-1 autocorrelation
    along t and f (1/sqrt n'), E|z|^4 - 2 (sqrt 20 / sqrt n), cross-correlation between seeds and between draws (1/sqrt n)."""
    T = 256
    z = _fill(SEEDS, F, T, 0, 2).cpu().numpy().astype(np.complex128)
    P = {(s, d): z[d, b, 0] for d in range(2) for b, s in enumerate(SEEDS)}
    n = F * T
    se = 1 / np.sqrt(n)
    stats = {}
    for k, p in P.items():
        assert np.abs(p).max() <= 4.09
        re, im = p.real * np.sqrt(2), p.imag * np.sqrt(2)
        stats[k + ("mean_re",)] = re.mean() / se
        stats[k + ("mean_im",)] = im.mean() / se
        stats[k + ("var_re",)] = (re.var() - 1) / (np.sqrt(2) * se)
        stats[k + ("var_im",)] = (im.var() - 1) / (np.sqrt(2) * se)
        stats[k + ("cov",)] = (re * im).mean() / se
        for name, c in (("re", re), ("im", im)):
            stats[k + ("lag_t_" + name,)] = (c[:, 1:] * c[:, :-1]).mean() * np.sqrt(c[:, 1:].size)
            stats[k + ("lag_f_" + name,)] = (c[1:] * c[:-1]).mean() * np.sqrt(c[1:].size)
        stats[k + ("m4",)] = ((np.abs(p) ** 4).mean() - 2) / (np.sqrt(20) * se)
    pairs = [((SEEDS[0], d), (SEEDS[1], d), "seeds") for d in range(2)] + [((s, 0), (s, 1), "draws") for s in SEEDS]
    for a, b, what in pairs:
        stats[a + b + (what + "_re",)] = (P[a].real * P[b].real).mean() * 2 / se
        stats[a + b + (what + "_im",)] = (P[a].imag * P[b].imag).mean() * 2 / se
    worst = max(stats, key=lambda k: abs(stats[k]))
    print(f"seeded noise: {len(stats)} statistics, the largest |z-score| = {abs(stats[worst]):.2f} at {worst}")
    bad = {k: round(float(v), 2) for k, v in stats.items() if not abs(v) <= 4}
    assert not bad, bad


# ---- 4. seeded == filled, bit for bit ---------------------------------------------------------------------------------
@pytest.mark.parametrize("nf", [8, 64])
@pytest.mark.parametrize("precision", ["bf16", "fp32"])
@pytest.mark.parametrize("solver", ["euler", "midpoint"])
def test_enhance_seeded_equals_filled(nf, precision, solver):
    """fd_enhance_seeded(seeds) == fd_enhance(noise = fd_noise_fill(seeds)), eager and as a captured graph (2 x 1 s)."""
    m = _flow(nf, precision)
    y = _wave(2, 48000, seed=3)
    seeds = [11, (1 << 63) + 12]
    Fm, Tp = _frames(m, 48000)
    nz = _fill(seeds, Fm, Tp)[0]
    ref = m.enhance(y, N=2, solver=solver, noise=nz, use_graph=False)
    assert torch.isfinite(ref).all() and ref.abs().max() > 0
    assert torch.equal(m.enhance(y, N=2, solver=solver, seed=seeds, use_graph=False), ref), "eager: seeded != filled"
    for i in range(3):    # eager at first sight, captured at the second, replayed at the third
        assert torch.equal(m.enhance(y, N=2, solver=solver, seed=seeds, use_graph=True), ref), f"graph call {i}: seeded != filled"
        assert torch.equal(m.enhance(y, N=2, solver=solver, noise=nz, use_graph=True), ref), f"graph call {i}: filled"
    # every solver state (fd_ode_solve_seeded with traj)
    ta, wa = m.enhance(y, N=2, solver=solver, seed=seeds, return_traj=True)
    tb, wb = m.enhance(y, N=2, solver=solver, noise=nz, return_traj=True)
    assert torch.equal(torch.view_as_real(ta), torch.view_as_real(tb)) and all(torch.equal(a, b) for a, b in zip(wa, wb))


def _score(kind, precision):
    if kind == "1x1":
        from test_hip_baselines import baseline
        return baseline("score", precision)
    from test_hip_sgmse import make_model
    return make_model(8, precision, preset="score_model_sgmse")


@pytest.mark.parametrize("kind", ["1x1", "3x3"])
@pytest.mark.parametrize("predictor", ["reverse_diffusion", "euler_maruyama"])
@pytest.mark.parametrize("corrector", ["ald", "none"])
def test_score_enhance_seeded_equals_filled(kind, predictor, corrector):
    """fd_score_enhance_seeded == fd_score_enhance on n_draws filled planes: nf = 8, N = 4, both output-layer sizes."""
    m = _score(kind, "bf16")
    L = 12000
    y = _wave(2, L, seed=4)
    seeds = [21, 22]
    Fm, Tp = _frames(m, L)
    kw = dict(N=4, predictor=predictor, corrector=corrector, corrector_steps=1, snr=0.5)
    n = m.num_draws(4, predictor, corrector, 1)
    nz = _fill(seeds, Fm, Tp, 0, n)
    for use_graph in (False, True):
        ref = m.enhance(y, noise=nz, use_graph=use_graph, **kw)
        out = m.enhance(y, seed=seeds, use_graph=use_graph, **kw)
        assert torch.isfinite(ref).all() and ref.abs().max() > 0
        assert torch.equal(out, ref), f"use_graph={use_graph}: seeded != filled"
    shifted = m.enhance(y, noise=_fill(seeds, Fm, Tp, 1, n), use_graph=False, **kw)     # the draw indices matter
    assert not torch.equal(shifted, ref)


# ---- 5. placement invariance -------------------------------------------------------------------------------------------
def test_fill_does_not_depend_on_width_or_batch():
    a = _fill(SEEDS, F, 256, 0, 2)
    b = _fill(SEEDS, F, 128, 0, 2)
    assert torch.equal(torch.view_as_real(a[..., :128]), torch.view_as_real(b))
    one = _fill(SEEDS[1:], F, 256, 1, 1)
    assert torch.equal(torch.view_as_real(one[0, 0]), torch.view_as_real(a[1, 1]))


def test_clip_alone_equals_batch_and_ragged_bucket():
    m = _flow(8, "bf16")
    L = 30000
    clip = _wave(1, L, seed=5)
    s = 0xDEADBEEFCAFEF00D
    alone = m.enhance(clip, N=2, solver="midpoint", seed=[s], use_graph=False)
    batch = torch.cat([_wave(2, L, seed=6), clip, _wave(1, L, seed=7)])
    out = m.enhance(batch, N=2, solver="midpoint", seed=[1, 2, s, 4], use_graph=False)
    assert torch.equal(out[2:3], alone), "position 3 of 4 != alone"
    others = [torch.from_numpy((0.1 * np.random.default_rng(9 + i).standard_normal(n)).astype(np.float32)) for i, n in enumerate((24576, 49151, 41234))]
    outs = m.enhance_batch([others[0], clip.reshape(-1), others[1], others[2]], N=2, solver="midpoint", seeds=[5, s, 6, 7])
    assert torch.equal(outs[1], alone.reshape(-1)), "ragged bucket != alone"
    again = m.enhance_batch([clip.reshape(-1), others[2]], N=2, solver="midpoint", seeds=torch.tensor([s - (1 << 64), 9]))
    assert torch.equal(again[0], alone.reshape(-1)), "int64 tensor seeds"


_SHARDED = r'''
import os, sys, numpy as np, torch, torch.distributed as dist
sys.path.insert(0, sys.argv[1])
import flowdec_amd
from flowdec_amd.dist import sharded_enhance
from flowdec_amd.noise import clip_seed
from oracle import flowdec_oracle as O
torch.cuda.set_device(0)
dist.init_process_group("gloo", rank=int(os.environ["RANK"]), world_size=2)
m = flowdec_amd.from_preset("flowdec_75m", precision="bf16", nf=8)
m.load_state_dict({k: torch.from_numpy(v) for k, v in O.random_state_dict(seed=8, nf=8).items()}, strict=False)
m = m.cuda()
y = torch.from_numpy((0.1 * np.random.default_rng(5).standard_normal((3, 1, 24000))).astype(np.float32)).cuda()
out = sharded_enhance(m, y, N=2, solver="midpoint", seed=77, rng="native")          # 2 + 1 clips
assert out.shape == y.shape and torch.isfinite(out).all()
assert torch.equal(out, m.enhance(y, N=2, solver="midpoint", seed=77)), "sharded != unsharded"
for i in range(3):
    one = m.enhance(y[i:i + 1], N=2, solver="midpoint", seed=[clip_seed(77, i)])
    assert torch.equal(out[i:i + 1], one), f"clip {i}: in a shard != alone"
auto = sharded_enhance(m, y, N=2, solver="midpoint", rng="native")                  # rank 0's seed, broadcast
assert torch.isfinite(auto).all() and not torch.equal(auto, out)
dist.barrier(); dist.destroy_process_group()
print("rank ok")
'''


def test_sharded_native_rng_two_ranks_one_gpu(tmp_path):
    script = tmp_path / "native2.py"
    script.write_text(_SHARDED)
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    env.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0", WORLD_SIZE="2")
    procs = [subprocess.Popen([sys.executable, str(script), ROOT], env=dict(env, RANK=str(r)), stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
             for r in range(2)]
    outs = [p.communicate(timeout=900)[0].decode() for p in procs]
    assert all(p.returncode == 0 for p in procs), "\n".join(o[-3000:] for o in outs)
    assert all("rank ok" in o for o in outs)


# ---- 6. graph replay with changing seeds --------------------------------------------------------------------------------
def test_graph_replay_reads_new_seeds():
    m = _flow(8, "bf16")
    y = _wave(2, 24000, seed=8)
    first = [m.enhance(y, N=2, solver="euler", seed=[31, 32], use_graph=True) for _ in range(3)]     # captured at the second call
    assert torch.equal(first[0], first[1]) and torch.equal(first[0], first[2])
    ptr = m._io[next(iter(m._io))]["seeds"].data_ptr()
    new = m.enhance(y, N=2, solver="euler", seed=[41, 42], use_graph=True)                           # replay: same pointer, new contents
    assert m._io[next(iter(m._io))]["seeds"].data_ptr() == ptr
    assert torch.equal(new, m.enhance(y, N=2, solver="euler", seed=[41, 42], use_graph=False))
    assert not torch.equal(new, first[0])


# ---- 7. Python surface -------------------------------------------------------------------------------------------------
def test_flow_enhance_seed_argument():
    from flowdec_amd.noise import clip_seed
    m = _flow(8, "fp32")
    y = _wave(2, 12000, seed=9)
    a = m.enhance(y, N=2, solver="midpoint", seed=5)
    assert torch.equal(a, m.enhance(y, N=2, solver="midpoint", seed=5))
    assert not torch.equal(a, m.enhance(y, N=2, solver="midpoint", seed=6))
    assert torch.equal(a, m.enhance(y, N=2, solver="midpoint", seed=[clip_seed(5, 0), clip_seed(5, 1)]))
    assert torch.equal(a, m.enhance(y, N=2, solver="midpoint", seed=torch.tensor([clip_seed(5, 0), clip_seed(5, 1)], dtype=torch.uint64)))
    assert torch.equal(m.enhance(y[0, 0], N=2, solver="midpoint", seed=5), a[0, 0])            # 1-D input, clip 0
    # the adaptive solver: the initial plane comes from fd_noise_fill, then the unseeded call
    Fm, Tp = _frames(m, 12000)
    nz = _fill([clip_seed(5, 0), clip_seed(5, 1)], Fm, Tp)[0]
    d1 = m.enhance(y, N=2, solver="dopri5", seed=5, atol=1e-2, rtol=1e-2)
    assert torch.equal(d1, m.enhance(y, N=2, solver="dopri5", noise=nz, atol=1e-2, rtol=1e-2))


def test_score_enhance_seed_allocates_no_noise():
    m = _score("1x1", "bf16")
    y = _wave(2, 12000, seed=10)
    kw = dict(N=3, predictor="reverse_diffusion", corrector="ald")
    a = m.enhance(y, seed=5, **kw)
    io = m._io[next(iter(m._io))]
    assert io["noise"] is None and io["seeds"] is not None
    assert torch.equal(a, m.enhance(y, seed=5, **kw)) and not torch.equal(a, m.enhance(y, seed=6, **kw))
    Fm, Tp = _frames(m, 12000)
    from flowdec_amd.noise import clip_seed
    z0 = _fill([clip_seed(5, 0), clip_seed(5, 1)], Fm, Tp)[0]
    o1 = m.enhance(y, sampler_type="ode", N=30, rtol=1e-2, atol=1e-2, seed=5)
    assert torch.equal(o1, m.enhance(y, sampler_type="ode", N=30, rtol=1e-2, atol=1e-2, noise=z0))


def test_cli_native_rng_does_not_depend_on_batching(tmp_path):
    from test_cli import synthetic_ckpt
    from flowdec_amd import enhance_cli
    torch.save(synthetic_ckpt(), tmp_path / "m.ckpt")
    ind = tmp_path / "in"
    ind.mkdir()
    rng = np.random.default_rng(2)
    spec = [("a", 30000), ("b", 41234), ("c", 24576), ("d", 49151), ("e", 20000), ("f", 23000)]
    for name, n in spec:
        enhance_cli.save_wav(str(ind / f"{name}.wav"), torch.from_numpy((0.1 * rng.standard_normal((1, n))).astype(np.float32)), 48000)
    common = ["--ckpt", str(tmp_path / "m.ckpt"), "--files", str(ind), "--N", "2", "--solver", "midpoint", "--rng", "native"]
    r8 = enhance_cli.run(common + ["--seed", "3", "--outdir", str(tmp_path / "o8"), "--batch-files", "8"])
    r1 = enhance_cli.run(common + ["--seed", "3", "--outdir", str(tmp_path / "o1"), "--batch-files", "1"])
    r4 = enhance_cli.run(common + ["--seed", "4", "--outdir", str(tmp_path / "o4"), "--batch-files", "8"])
    assert r8.n_done == r1.n_done == r4.n_done == len(spec)
    for name, _ in spec:
        a = (tmp_path / "o8" / f"{name}.wav").read_bytes()
        assert a == (tmp_path / "o1" / f"{name}.wav").read_bytes(), f"{name}.wav: batched output differs from the one-file-per-call output"
        assert a != (tmp_path / "o4" / f"{name}.wav").read_bytes(), f"{name}.wav: --seed has no effect"
    assert enhance_cli.run(common + ["--outdir", str(tmp_path / "o0")]).n_done == len(spec)     # no --seed: one is drawn and printed


# ---- 8. nothing moved: the torch routes give the bits of the commit before the seeded path ------------------------------------
@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_torch_noise_routes_unchanged(precision):
    """enhance(generator=) and sharded_enhance(seed=) (rng='torch') against waveforms recorded on an MI355X from the build that preceded
    the seeded path (tests/golden/g31_torch_noise_parent.npz: 3 x 12000 samples, nf = 8, midpoint N = 2)."""
    from flowdec_amd.dist import sharded_enhance
    g = load_golden("g31_torch_noise_parent.npz")
    m = _flow(8, precision)
    y = torch.from_numpy(g["y"]).cuda()
    a = m.enhance(y, N=2, solver="midpoint", generator=torch.Generator(device="cuda").manual_seed(7))
    assert np.array_equal(a.cpu().numpy(), g[f"generator7_{precision}"])
    b = sharded_enhance(m, y, N=2, solver="midpoint", seed=99)
    assert np.array_equal(b.cpu().numpy(), g[f"sharded_seed99_{precision}"])
