"""Ragged batches of the ScoreDec and regression baselines: ScoreModel.enhance_batch / RegressionModel.enhance_batch
(fd_score_enhance_ragged / fd_regression_enhance_ragged) and the command line on their checkpoints.

The contract is the one FlowModel.enhance_batch has (tests/test_hip_ragged.py): every clip of a ragged batch is BIT-IDENTICAL to the
one-clip call on that clip with the same noise -- which G13 pins to the reference's ScoreModel / RegressionModel (here again, inside a
ragged batch).  The reference's driver runs these classes file by file (enhance.py:66,96-137)."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import load_golden
from test_cli import synthetic_ckpt
from test_hip_baselines import TOL_REGRESSION, TOL_SCORE, baseline, golden_noise
from test_hip_ops import check
from test_oracle_golden import SCORE_CASES

pytestmark = pytest.mark.gpu

HOP, NFFT, F, TP = 384, 1534, 768, 64
# one T_pad = 64 bucket (T = 1 + L // 384 <= 64 <=> L <= 24575); clips 0 and 1 are G13's
LENS_A = [12000, 12000, 20000, 1000]
# another length set of the same bucket, with both of its ends: 768 is the shortest clip the reflect padding takes, 24575 the longest
LENS_B = [768, 24575, 12000, 5000]


def test_the_clips_share_one_bucket():
    from flowdec_amd import _lib as L
    lib = L.load()
    for n in LENS_A + LENS_B:
        assert lib.fd_padded_frames(lib.fd_num_frames(n, HOP)) == TP, n
    assert lib.fd_padded_frames(lib.fd_num_frames(24576, HOP)) == 2 * TP


def clips_of(lengths, seed):
    """LENS_A: G13's two clips, then random ones; any other set: random clips."""
    rng = np.random.default_rng(seed)
    out = [torch.from_numpy((0.1 * (1 + i) * rng.standard_normal(n)).astype(np.float32)) for i, n in enumerate(lengths)]
    if lengths is LENS_A:
        g = load_golden("g13_score_nf8.npz")
        out[0], out[1] = torch.from_numpy(g["y"][0, 0].copy()), torch.from_numpy(g["y"][1, 0].copy())
    return out


def noises_of(lengths, n, seed):
    """One [n, 1, 1, F, TP] complex plane stack per clip; LENS_A's first two are the planes of the G13 fixture."""
    gen = torch.Generator().manual_seed(seed)
    out = [torch.view_as_complex(torch.randn(n, 1, 1, F, TP, 2, generator=gen) / np.sqrt(2)) for _ in lengths]
    if lengths is LENS_A:
        nz = golden_noise(load_golden("g13_score_nf8.npz"), n)      # [n, 2, 1, F, TP]
        out[0], out[1] = nz[:, 0:1], nz[:, 1:2]
    return out


def assert_all_equal(outs, refs, what):
    assert len(outs) == len(refs)
    for b, (o, r) in enumerate(zip(outs, refs)):
        assert o.shape == r.shape and o.device == r.device
        assert torch.isfinite(r).all() and r.abs().max() > 0
        assert torch.equal(o, r), f"{what}: clip {b} ({r.numel()} samples) differs from the one-clip call"


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("case", list(SCORE_CASES))
def test_score_enhance_batch_bit_identical_and_on_the_golden(case, prec):
    from flowdec_amd.noise import clip_seed
    g = load_golden("g13_score_nf8.npz")
    m = baseline("score", prec)
    kw = dict(SCORE_CASES[case])
    n = m.num_draws(kw["N"], kw["predictor"], kw["corrector"], kw.get("corrector_steps", 1))
    sets = {"A": (clips_of(LENS_A, 1), noises_of(LENS_A, n, 2)), "B": (clips_of(LENS_B, 3), noises_of(LENS_B, n, 4))}
    # -- injected noise planes: the one-clip calls first, then the batch calls back to back (they share one set of staging buffers, so
    # the second sighting of the key captures the graph and the later ones replay it)
    ref = {k: [m.enhance(c, noise=z, use_graph=False, **kw) for c, z in zip(*cz)] for k, cz in sets.items()}
    clips, nz = sets["A"]
    eager = m.enhance_batch(clips, noise=nz, use_graph=False, **kw)
    assert_all_equal(eager, ref["A"], "eager")
    first = m.enhance_batch(clips, noise=nz, use_graph=True, **kw)          # first sighting of the key: runs eagerly
    captured = m.enhance_batch(clips, noise=nz, use_graph=True, **kw)       # second sighting: captured, then launched
    assert_all_equal(first, ref["A"], "first graph call")
    assert_all_equal(captured, ref["A"], "captured graph")
    replay_b = m.enhance_batch(sets["B"][0], noise=sets["B"][1], use_graph=True, **kw)   # replay: other contents of `lengths`
    assert_all_equal(replay_b, ref["B"], "graph replay with other lengths")
    replay_a = m.enhance_batch(clips, noise=nz, use_graph=True, **kw)
    assert_all_equal(replay_a, ref["A"], "graph replay")
    # -- the reference's result inside the ragged batch: clips 0 and 1 are G13's y with G13's noise planes
    check(f"ragged score_{case}[{prec}]", torch.stack([eager[0], eager[1]])[:, None].numpy(), g[case], TOL_SCORE[prec])
    # -- one torch.Generator per clip
    gens = lambda: [torch.Generator(device="cuda").manual_seed(40 + b) for b in range(len(clips))]
    ref_g = [m.enhance(c, generator=gb, use_graph=False, **kw) for c, gb in zip(clips, gens())]
    assert_all_equal(m.enhance_batch(clips, generator=gens(), **kw), ref_g, "generators")
    assert not torch.equal(ref_g[2], ref["A"][2])
    # -- the library's own seeded noise
    seeds = [clip_seed(9, b) for b in range(len(clips))]
    ref_s = [m.enhance(c, seed=[s], use_graph=False, **kw) for c, s in zip(clips, seeds)]
    assert_all_equal(m.enhance_batch(clips, seeds=seeds, use_graph=False, **kw), ref_s, "seeds, eager")
    for call in ("first", "captured", "replay"):
        assert_all_equal(m.enhance_batch(clips, seeds=seeds, **kw), ref_s, f"seeds, {call}")


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_regression_enhance_batch_bit_identical_and_on_the_golden(prec):
    g = load_golden("g13_score_nf8.npz")
    m = baseline("regression", prec)
    a, b = clips_of(LENS_A, 1), clips_of(LENS_B, 3)
    ref_a, ref_b = [m.enhance(c, use_graph=False) for c in a], [m.enhance(c, use_graph=False) for c in b]
    eager = m.enhance_batch(a, use_graph=False)
    assert_all_equal(eager, ref_a, "eager")
    assert_all_equal(m.enhance_batch(a), ref_a, "first graph call")
    assert_all_equal(m.enhance_batch(a), ref_a, "captured graph")
    assert_all_equal(m.enhance_batch(b), ref_b, "graph replay with other lengths")
    assert_all_equal(m.enhance_batch(a), ref_a, "graph replay")
    check(f"ragged regression[{prec}]", torch.stack([eager[0], eager[1]])[:, None].numpy(), g["regression"], TOL_REGRESSION[prec])
    # shapes and devices follow the clips
    outs = m.enhance_batch([a[0][None].cuda(), a[2][None, None]])
    assert outs[0].shape == (1, 12000) and outs[0].is_cuda and outs[1].shape == (1, 1, 20000) and not outs[1].is_cuda
    assert torch.equal(outs[0][0].cpu(), ref_a[0]) and torch.equal(outs[1][0, 0], ref_a[2])
    assert m.enhance_batch([]) == []


def _rows(clips, Lrow):
    y = torch.zeros(len(clips), Lrow)
    for b, c in enumerate(clips):
        y[b, :c.numel()] = c
    return y.cuda()


def test_native_ragged_calls_zero_the_tail_and_equal_the_plain_calls():
    """Through ctypes: a row of x_hat is zero from lengths[b] on (the buffer is poisoned first), and with every length equal to L the
    ragged entry points are fd_score_enhance / fd_score_enhance_seeded / fd_regression_enhance."""
    from flowdec_amd import _lib as L
    lib = L.load()
    kw = SCORE_CASES["rd_ald_N3"]
    cfg = None
    for kind in ("score", "regression"):
        m = baseline(kind, "bf16")
        h = m._sync_native()
        if kind == "score":
            cfg = L.FdScoreConfig(m.sde.theta, m.sde.sigma_min, m.sde.sigma_max, m.t_eps, kw["snr"], kw["N"], 0, 0, 1, 1)
            n = lib.fd_score_num_draws(C.byref(cfg))
        # (a) ragged rows of the bucket's row length
        Lrow = HOP * TP - 1
        y = _rows(clips_of(LENS_A, 1), Lrow)
        lens = torch.tensor(LENS_A, dtype=torch.int32, device="cuda")
        seeds = torch.arange(11, 15, dtype=torch.int64, device="cuda")
        ws = torch.empty(lib.fd_enhance_workspace_bytes(h, 4, Lrow), dtype=torch.uint8, device="cuda")
        out = torch.full((4, Lrow), float("nan"), device="cuda")
        if kind == "score":
            L.check(lib.fd_score_enhance_ragged(h, L.ptr(y), L.ptr(lens), None, L.ptr(seeds), C.byref(cfg), L.ptr(out), 4, Lrow, L.ptr(ws),
                                                ws.numel(), 0, L.stream()))
        else:
            L.check(lib.fd_regression_enhance_ragged(h, L.ptr(y), L.ptr(lens), L.ptr(out), 4, Lrow, L.ptr(ws), ws.numel(), 0, L.stream()))
        torch.cuda.synchronize()
        for b, l in enumerate(LENS_A):
            assert torch.isfinite(out[b, :l]).all() and out[b, :l].abs().max() > 0
            assert not out[b, l:].any(), f"{kind}: clip {b}: samples behind its {l} must be zero"
        # (b) equal lengths: the plain entry points
        Lw = 12000
        y = _rows(clips_of([Lw, Lw, Lw], 5), Lw)
        lens = torch.full((3,), Lw, dtype=torch.int32, device="cuda")
        ws = torch.empty(lib.fd_enhance_workspace_bytes(h, 3, Lw), dtype=torch.uint8, device="cuda")
        got, want = torch.full((3, Lw), float("nan"), device="cuda"), torch.full((3, Lw), float("nan"), device="cuda")
        tail = (3, Lw, L.ptr(ws), ws.numel(), 0, L.stream())
        if kind == "score":
            nz = torch.view_as_real(torch.randn(n, 3, 1, F, TP, dtype=torch.complex64, device="cuda")).contiguous()
            L.check(lib.fd_score_enhance(h, L.ptr(y), L.ptr(nz), C.byref(cfg), L.ptr(want), *tail))
            L.check(lib.fd_score_enhance_ragged(h, L.ptr(y), L.ptr(lens), L.ptr(nz), None, C.byref(cfg), L.ptr(got), *tail))
            torch.cuda.synchronize()
            assert torch.isfinite(want).all() and torch.equal(got, want), "fd_score_enhance_ragged(noise) != fd_score_enhance"
            L.check(lib.fd_score_enhance_seeded(h, L.ptr(y), L.ptr(seeds), C.byref(cfg), L.ptr(want), *tail))
            L.check(lib.fd_score_enhance_ragged(h, L.ptr(y), L.ptr(lens), None, L.ptr(seeds), C.byref(cfg), L.ptr(got), *tail))
        else:
            L.check(lib.fd_regression_enhance(h, L.ptr(y), L.ptr(want), *tail))
            L.check(lib.fd_regression_enhance_ragged(h, L.ptr(y), L.ptr(lens), L.ptr(got), *tail))
        torch.cuda.synchronize()
        assert torch.isfinite(want).all() and want.abs().max() > 0 and torch.equal(got, want), f"{kind}: ragged with equal lengths != the plain call"


def test_normfac_slot_of_the_enhance_workspace():
    """The workspace layout Y | X | normfac[B] | rest from outside: fd_enhance_normfac_offset is two 256-byte-aligned complex64 states
    [B][F][T_pad], and after fd_enhance the four bytes per clip found there are the clips' maxima as ops.stft_compress takes them."""
    from flowdec_amd import _lib as L, ops
    from test_hip_noise import _flow
    lib = L.load()
    m = _flow(8, "bf16")
    h = m._sync_native()
    B, Lw = 2, 12000
    fd_align = lambda n: (n + 255) // 256 * 256
    off = lib.fd_enhance_normfac_offset(h, B, Lw)
    assert off == 2 * fd_align(8 * B * F * TP)
    need = lib.fd_enhance_workspace_bytes(h, B, Lw)
    assert need > off + 4 * B
    y = _rows(clips_of([Lw, Lw], 6), Lw)
    nz = torch.view_as_real(torch.randn(B, 1, F, TP, dtype=torch.complex64, device="cuda")).contiguous()
    ws = torch.zeros(need, dtype=torch.uint8, device="cuda")
    out = torch.full((B, Lw), float("nan"), device="cuda")
    L.check(lib.fd_enhance(h, L.ptr(y), L.ptr(nz), 1.0, 2, L.SOLVERS["euler"], L.ptr(out), B, Lw, L.ptr(ws), ws.numel(), 0, L.stream()))
    _, normfac, _ = ops.stft_compress(y, normalize=True, **m.feature_extractor._cfg())
    torch.cuda.synchronize()
    assert torch.isfinite(out).all() and normfac.shape == (B,) and normfac[0] != normfac[1] and normfac.min() > 0
    assert torch.equal(ws[off:off + 4 * B].view(torch.float32), normfac)


@pytest.mark.parametrize("kind", ["flow", "score", "regression"])
def test_one_resident_staging_entry(kind):
    """The staging buffers of the three classes (`model._io`: one resident shape): a seeded call allocates no noise plane, a repeated call
    finds every buffer where it was (a captured graph is keyed on the addresses), seeded and unseeded calls of one shape share y and out,
    and a ragged batch leaves one entry behind."""
    from test_hip_noise import _flow
    m = _flow(8, "bf16") if kind == "flow" else baseline(kind, "bf16")
    kw = {"flow": dict(N=2, solver="euler"), "score": dict(N=2), "regression": {}}[kind]
    random = kind != "regression"
    y = torch.stack(clips_of([12000, 12000], 7))[:, None]

    def ptrs():
        assert len(m._io) == 1
        io = m._io[next(iter(m._io))]
        return {k: None if io[k] is None else io[k].data_ptr() for k in ("y", "out", "seeds", "noise")}

    # -- a seeded call: seeds, and no noise plane; the repeat finds the same addresses
    m._io = {}
    sd = dict(seed=[21, 22]) if random else {}
    s0 = m.enhance(y, **sd, **kw)
    p = ptrs()
    assert p["noise"] is None and (p["seeds"] is not None) == random and p["y"] is not None and p["out"] is not None
    assert torch.equal(m.enhance(y, **sd, **kw), s0) and ptrs() == p
    if random:
        # -- unseeded, then seeded, then unseeded again at one shape: y, out (and the seeds, once they exist) stay in place; the seeded
        # call lets the noise plane go
        m._io = {}
        gen = lambda: torch.Generator(device="cuda").manual_seed(3)
        u0 = m.enhance(y, generator=gen(), **kw)
        p = ptrs()
        assert p["noise"] is not None and p["seeds"] is None
        assert torch.equal(m.enhance(y, generator=gen(), **kw), u0) and ptrs() == p          # the second sighting of the key: captured
        s1 = m.enhance(y, **sd, **kw)
        q = ptrs()
        assert q["noise"] is None and q["seeds"] is not None and (q["y"], q["out"]) == (p["y"], p["out"])
        u1 = m.enhance(y, generator=gen(), **kw)
        r = ptrs()
        assert r["noise"] is not None and (r["y"], r["out"], r["seeds"]) == (q["y"], q["out"], q["seeds"])
        assert torch.equal(u1, u0) and torch.equal(s1, s0) and not torch.equal(u0, s0)
        assert torch.equal(u0, m.enhance(y, generator=gen(), use_graph=False, **kw)) and ptrs() == r
        assert torch.equal(s1, m.enhance(y, use_graph=False, **sd, **kw))
    # -- a ragged batch of one T_pad = 64 bucket: one resident shape (rows, row length), every clip equal to its one-clip call
    clips = clips_of([12000, 20000], 8)
    outs = m.enhance_batch(clips, **(dict(seeds=[31, 32]) if random else {}), **kw)
    ptrs()
    assert next(iter(m._io))[:2] == (2, HOP * TP - 1)
    assert_all_equal(outs, [m.enhance(c, **(dict(seed=[s]) if random else {}), **kw) for c, s in zip(clips, [31, 32])], kind)


def test_enhance_batch_errors():
    s, r = baseline("score", "bf16"), baseline("regression", "bf16")
    clips = clips_of(LENS_A, 1)
    for m in (s, r):
        with pytest.raises(RuntimeError, match="bucket"):
            m.enhance_batch([clips[0], torch.zeros(30000)])
        with pytest.raises(RuntimeError, match="samples"):
            m.enhance_batch([clips[0], torch.zeros(NFFT // 2)])        # not longer than the reflect padding
        with pytest.raises(RuntimeError, match=r"\[L\]"):
            m.enhance_batch([torch.zeros(2, 12000)])
    with pytest.raises(ValueError, match="ode"):
        s.enhance_batch(clips, sampler_type="ode", N=2)
    with pytest.raises(ValueError):
        s.enhance_batch(clips, corrector="bogus", N=2)
    n = s.num_draws(2)
    with pytest.raises(RuntimeError, match="per clip"):
        s.enhance_batch(clips, N=2, noise=noises_of(LENS_A, n, 2)[:3])
    with pytest.raises(RuntimeError, match="per clip"):
        s.enhance_batch(clips, N=2, generator=[torch.Generator(device="cuda") for _ in range(3)])
    with pytest.raises(RuntimeError):
        s.enhance_batch(clips, N=2, seeds=[1, 2, 3])
    with pytest.raises(RuntimeError):                                     # planes for another N
        s.enhance_batch(clips, N=3, noise=noises_of(LENS_A, n, 2))


# ------------------------------------------------------------------------------------------------
# the command line
# ------------------------------------------------------------------------------------------------
SPEC = [("a", 12000), ("b", 20000), ("c", 30000), ("d", 12000), ("e", 30000), ("f", 20000)]   # two buckets: T_pad 64 (a b d f), 128 (c e)


def corpus(tmp_path, target, **hp):
    from flowdec_amd import enhance_cli
    ckpt = synthetic_ckpt()
    if target:
        ckpt["hyper_parameters"]["model"]["_target_"] = target
    ckpt["hyper_parameters"]["model"].update(hp)
    for sd in (ckpt["state_dict"], ckpt["_pl_ema_state_dict"]):     # G13's output scale: keeps a sampler on random weights in range
        sd["backbone.output_layer.weight"] = sd["backbone.output_layer.weight"] * 0.02
    torch.save(ckpt, tmp_path / "m.ckpt")
    ind = tmp_path / "in"
    ind.mkdir()
    rng = np.random.default_rng(2)
    for name, n in SPEC:
        enhance_cli.save_wav(str(ind / f"{name}.wav"), torch.from_numpy((0.1 * rng.standard_normal((1, n))).astype(np.float32)), 48000)
    return ["--ckpt", str(tmp_path / "m.ckpt"), "--files", str(ind)]


def run_cli(tmp_path, common, name, extra):
    from flowdec_amd import enhance_cli
    res = enhance_cli.run(common + ["--outdir", str(tmp_path / name)] + extra)
    assert res.n_done == len(SPEC)
    return {n: (tmp_path / name / f"{n}.wav").read_bytes() for n, _ in SPEC}


def test_cli_scoredec_checkpoint(tmp_path, capsys):
    from flowdec_amd import ScoreModel, enhance_cli
    common = corpus(tmp_path, "flowdec.model.ScoreModel", sde=dict(_target_="flowdec.sdes.OUVESDE", theta=1.5, sigma_min=0.05, sigma_max=0.5, N=30),
                    t_eps=0.03)
    sampler = ["--N", "2", "--predictor", "reverse_diffusion", "--corrector", "ald", "--snr", "0.5"]
    o8 = run_cli(tmp_path, common, "o8", sampler + ["--seed", "11", "--batch-files", "8"])
    assert "model=ScoreModel" in capsys.readouterr().out
    o1 = run_cli(tmp_path, common, "o1", sampler + ["--seed", "11", "--batch-files", "1"])
    n8 = run_cli(tmp_path, common, "n8", sampler + ["--seed", "11", "--rng", "native", "--batch-files", "8"])
    n1 = run_cli(tmp_path, common, "n1", sampler + ["--seed", "11", "--rng", "native", "--batch-files", "1"])
    for name, _ in SPEC:
        assert o8[name] == o1[name], f"{name}.wav: batched output differs from the one-file-per-call output (--seed)"
        assert n8[name] == n1[name], f"{name}.wav: batched output differs from the one-file-per-call output (--rng native)"
        assert o8[name] != n8[name]
    # file b is index 1 of the work list: its generator is seeded 11 + 1
    m = enhance_cli.load_from_checkpoint(str(tmp_path / "m.ckpt"), map_location="cuda:0")
    assert type(m) is ScoreModel and m.sde.sigma_max == 0.5
    y, _ = enhance_cli.load_wav(str(tmp_path / "in" / "b.wav"))
    ref = m.enhance(y, N=2, predictor="reverse_diffusion", corrector="ald", snr=0.5, generator=torch.Generator(device="cuda:0").manual_seed(12))
    got, sr = enhance_cli.load_wav(str(tmp_path / "o8" / "b.wav"))
    assert sr == 48000 and torch.equal(got, ref) and torch.isfinite(ref).all() and ref.abs().max() > 0
    # the sampler flags reach the model
    snr = run_cli(tmp_path, common, "snr", ["--N", "2", "--snr", "0.3", "--seed", "11"])
    none = run_cli(tmp_path, common, "none", ["--N", "2", "--corrector", "none", "--seed", "11"])
    em = run_cli(tmp_path, common, "em", ["--N", "2", "--predictor", "euler_maruyama", "--seed", "11"])
    solver = run_cli(tmp_path, common, "solver", sampler + ["--seed", "11", "--solver", "dopri5"])      # ignored, as in the reference
    for name, _ in SPEC:
        assert snr[name] != o8[name] and none[name] != o8[name] and em[name] != o8[name] and solver[name] == o8[name]


def test_cli_regression_checkpoint(tmp_path, capsys):
    from flowdec_amd import RegressionModel, enhance_cli
    common = corpus(tmp_path, "flowdec.model.RegressionModel")
    o8 = run_cli(tmp_path, common, "o8", ["--N", "1", "--batch-files", "8", "--seed", "3", "--rng", "native", "--rtf"])
    assert "model=RegressionModel" in capsys.readouterr().out
    o1 = run_cli(tmp_path, common, "o1", ["--N", "1", "--batch-files", "1"])
    assert o8 == o1
    rows = (tmp_path / "o8" / "rtfs.csv").read_text().strip().splitlines()
    assert rows[0] == "path,runtime,filetime,rtf" and len(rows) == 1 + len(SPEC)
    m = enhance_cli.load_from_checkpoint(str(tmp_path / "m.ckpt"), map_location="cuda:0")
    assert type(m) is RegressionModel
    y, _ = enhance_cli.load_wav(str(tmp_path / "in" / "c.wav"))
    got, _ = enhance_cli.load_wav(str(tmp_path / "o8" / "c.wav"))
    ref = m.enhance(y)
    assert torch.equal(got, ref) and ref.abs().max() > 0
    # the same weights as a score model give other audio: the class is not decoration
    sc = run_cli(tmp_path, common, "sc", ["--N", "2", "--model", "score", "--seed", "3"])
    assert all(sc[n] != o8[n] for n, _ in SPEC)


def test_cli_flow_checkpoint_is_unchanged_by_model_flag(tmp_path, capsys):
    common = corpus(tmp_path, None)
    args = ["--N", "2", "--solver", "midpoint", "--seed", "5", "--snr", "0.1", "--corrector", "none"]       # the score flags: ignored
    plain = run_cli(tmp_path, common, "plain", args)
    assert "model=FlowModel" in capsys.readouterr().out
    assert run_cli(tmp_path, common, "flag", args + ["--model", "flow"]) == plain
    assert run_cli(tmp_path, common, "one", ["--N", "2", "--solver", "midpoint", "--seed", "5", "--batch-files", "1"]) == plain
