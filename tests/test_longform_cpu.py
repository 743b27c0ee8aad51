"""Long-form planner and its host-side surroundings (flowdec_amd/longform.py; no GPU): the properties every plan must have, over the
lengths at which the construction changes shape; the cross-fade table against float64; the NumPy stitch; the CLI's argument errors."""
import numpy as np
import pytest

from flowdec_amd import longform
from flowdec_amd.longform import plan_rows, row_samples, stitch_reference, stitch_weights

HOP = 384
# (row_frames, halo_frames, xfade): the GPU tests' geometry, the defaults, no cross-fade, a cross-fade as wide as the halos allow, a hop of 1 below
GEOMETRIES = [(64, 8, 2 * HOP), (3712, 256, 2 * HOP), (64, 8, 0), (128, 2, 4 * HOP), (64, 0, 0)]


def check_plan(n, hop, rf, halo, xfade):
    rows = plan_rows(n, hop, rf, halo, xfade)
    W = row_samples(rf, hop)
    assert 1 + W // hop == rf and 1 + (W + 1) // hop == rf + 1, "W is the longest row that still has row_frames frames"
    ctx = (n, hop, rf, halo, xfade)
    if n <= W:
        assert rows == [longform.Row(0, n, 0, (0, n), None, None)], ctx
        return rows
    assert len(rows) >= 2, ctx
    for j, r in enumerate(rows):
        assert r.start % hop == 0 and r.frame0 * hop == r.start and r.start >= 0, (ctx, j)                 # the row's frame grid is the file's
        assert 0 < r.length <= W and r.start + r.length <= n, (ctx, j)
        assert -(-(1 + r.length // hop) // 64) * 64 == rf, (ctx, j, "every row pads to row_frames: one bucket")
        lo, hi = r.keep
        assert r.start <= lo < hi <= r.start + r.length, (ctx, j, "a row owns only samples it holds")
        assert lo == (0 if j == 0 else rows[j - 1].keep[1]), (ctx, j, "the kept ranges partition [0, n)")
        assert r.xfade_lo == (None if j == 0 else lo) and r.xfade_hi == (None if j == len(rows) - 1 else hi), (ctx, j)
    assert rows[-1].keep[1] == n and rows[-1].start + rows[-1].length == n, ctx
    for a, b in zip(rows, rows[1:]):
        c = b.xfade_lo                                                                                          # the boundary between a and b
        assert a.start < b.start, ctx
        for r in (a, b):                                                                                        # a halo of BOTH rows on EITHER side
            assert c - r.start >= halo * hop and r.start + r.length - c >= halo * hop, (ctx, c, r)
        assert a.start <= c - xfade // 2 and c + xfade // 2 <= a.start + a.length, (ctx, "the cross-fade lies inside the earlier row")
        assert b.start <= c - xfade // 2 and c + xfade // 2 <= b.start + b.length, (ctx, "... and inside the later row")
    for b, c in zip(rows[1:], rows[2:]):
        assert c.xfade_lo - b.xfade_lo >= xfade, (ctx, "cross-fades do not overlap")
    return rows


def edge_lengths(hop, rf, halo):
    W = row_samples(rf, hop)
    stride, first = (rf - 2 * halo - 1) * hop, (rf - halo - 1) * hop
    ns = {1, 2, hop, W - 1, W, W + 1, W + 2, W + hop - 1, W + hop, W + hop + 1}
    for k in (1, 2, 3, 7):
        full = k * stride + W                     # k + 1 whole rows end exactly here
        ns |= {full - 1, full, full + 1, full + 2, full + 5, full + hop - 1, full + hop, full + hop + 1}   # ... a last row shifted by < / = / > one hop
        bound = first + (k - 1) * stride          # the k-th boundary
        ns |= {bound - 1, bound, bound + 1, bound + halo * hop - 1, bound + halo * hop, bound + halo * hop + 1}
    return sorted(v for v in ns if v >= 1)


@pytest.mark.parametrize("rf,halo,xfade", GEOMETRIES)
def test_plan_properties_at_the_edges(rf, halo, xfade):
    for n in edge_lengths(HOP, rf, halo):
        check_plan(n, HOP, rf, halo, xfade)


@pytest.mark.parametrize("rf,halo,xfade", GEOMETRIES[:3])
def test_plan_properties_random_lengths(rf, halo, xfade):
    rng = np.random.default_rng(rf + halo)
    W = row_samples(rf, HOP)
    for n in rng.integers(1, 12 * W, size=300):
        check_plan(int(n), HOP, rf, halo, xfade)
    for hop in (1, 7, 256):                       # other frame grids
        for n in rng.integers(1, 6 * row_samples(rf, hop), size=40):
            check_plan(int(n), hop, rf, halo, min(xfade, 2 * halo * hop) // 2 * 2)


def test_plan_shapes():
    W = row_samples(64, HOP)
    assert len(plan_rows(W, HOP, 64, 8)) == 1 and len(plan_rows(W + 1, HOP, 64, 8)) == 2
    two = plan_rows(W + 1, HOP, 64, 8)
    assert two[1].start == HOP and two[1].length == W + 1 - HOP and two[1].frame0 == 1, "a last row shifted left to end at n, on the frame grid"
    assert two[0].keep == (0, 55 * HOP) and two[1].keep == (55 * HOP, W + 1)
    few = plan_rows(47 * HOP + W + 5, HOP, 64, 8)      # two whole rows and five samples: the third row starts one hop after the second
    assert [r.start for r in few] == [0, 47 * HOP, 48 * HOP] and few[2].length == W - HOP + 5
    # the defaults: an hour at 48 kHz
    hour = check_plan(3600 * 48000, HOP, 3712, 256, 2 * HOP)
    assert len(hour) == -(-(3600 * 48000 - row_samples(3712, HOP)) // ((3712 - 513) * HOP)) + 1 == 141
    assert plan_rows(10 ** 6, HOP) == plan_rows(10 ** 6, HOP, 3712, 256, 2 * HOP)


def test_plan_refuses_bad_geometry():
    for kw in (dict(row_frames=100), dict(row_frames=0), dict(xfade=3), dict(halo_frames=-1), dict(xfade=2 * 8 * HOP + 2),
               dict(halo_frames=32), dict(halo_frames=31, xfade=2 * HOP + 2)):
        args = dict(dict(row_frames=64, halo_frames=8, xfade=2 * HOP), **kw)
        with pytest.raises(ValueError):
            plan_rows(10 ** 6, HOP, **args)
    with pytest.raises(ValueError):
        plan_rows(0, HOP)
    assert len(plan_rows(1000, HOP, 64, 32)) == 1      # one row needs no room between halos


def test_stitch_weights_against_float64():
    for X in (2, 6, 2 * HOP, 4096):
        w = stitch_weights(X)
        assert w.dtype == np.float32 and w.shape == (X,)
        i = np.arange(X, dtype=np.float64)
        ref = 0.5 - 0.5 * np.cos(np.pi * (i + 0.5) / X)
        assert np.abs(w.astype(np.float64) - ref).max() <= 2.0 ** -25, "one rounding to float32 of a value in (0, 1)"
        assert np.all(np.diff(w) > 0) and 0 < w[0] and w[-1] < 1
        assert np.abs(w.astype(np.float64) + w[::-1].astype(np.float64) - 1).max() <= 2.0 ** -24, "w_i + w_(X-1-i) = 1: the fade is symmetric"
    assert stitch_weights(0).shape == (0,)


def test_stitch_reference():
    n, rf, halo, X = 3 * row_samples(64, HOP), 64, 8, 2 * HOP
    rows = plan_rows(n, HOP, rf, halo, X)
    rng = np.random.default_rng(0)
    x = rng.standard_normal(n).astype(np.float32)
    # rows that agree where they overlap stitch back to the file, exactly (a + w * 0)
    assert np.array_equal(stitch_reference([x[r.start:r.start + r.length] for r in rows], rows, X), x)
    # rows that differ by a constant: the copy regions are the owner's, the fade is a + w * (b - a) in float32
    outs = [x[r.start:r.start + r.length] + np.float32(j) for j, r in enumerate(rows)]
    got = stitch_reference(outs, rows, X)
    w = stitch_weights(X)
    for j, r in enumerate(rows):
        lo = r.keep[0] + (X // 2 if j else 0)
        hi = r.keep[1] - (X // 2 if j < len(rows) - 1 else 0)
        assert np.array_equal(got[lo:hi], x[lo:hi] + np.float32(j))
    c = rows[1].xfade_lo
    a, b = x[c - X // 2:c + X // 2], x[c - X // 2:c + X // 2] + np.float32(1)
    assert np.array_equal(got[c - X // 2:c + X // 2], a + w * (b - a))
    assert np.array_equal(stitch_reference(outs, rows, 0)[c - 1:c + 1], np.array([x[c - 1], x[c] + 1], dtype=np.float32))


def test_chunk_row_frames():
    f = longform.chunk_row_frames
    assert f(30.0, 48000, HOP) == 3712 and f(29.7, 48000, HOP) == 3712 and f(29.69, 48000, HOP) == 3648
    assert f(0.1, 48000, HOP) == 64 and f(1.0, 48000, HOP) == 64 and f(1.03, 48000, HOP) == 128
    assert longform.chunk_halo_frames(3712) == 256 and longform.chunk_halo_frames(1024) == 256 and longform.chunk_halo_frames(64) == 16


def test_symbols_and_python_surface():
    import inspect
    import flowdec_amd
    from flowdec_amd import _lib
    for name in ("fd_noise_fill_at", "fd_enhance_chunks", "fd_normfac", "fd_stitch_chunks"):
        assert name in _lib.SIGNATURES and hasattr(_lib.load(), name)
    sig = inspect.signature(flowdec_amd.FlowModel.enhance_long)
    want = dict(N=50, solver="euler", sigma_fac=1.0, seed=None, row_frames=3712, halo_frames=256, xfade=None, rows_per_call=8, use_graph=True)
    assert {k: p.default for k, p in sig.parameters.items() if k not in ("self", "y")} == want
    assert not hasattr(flowdec_amd.ScoreModel, "enhance_long") and not hasattr(flowdec_amd.RegressionModel, "enhance_long")
    m = flowdec_amd.from_preset("flowdec_75m", nf=8)
    with pytest.raises(ValueError, match="fixed-step"):
        m.enhance_long(np.zeros(10), solver="dopri5")
    # host-side refusals of the new entry points: nothing is launched
    lib = _lib.load()
    assert lib.fd_noise_fill_at(None, None, None, 1, 3, 64, 0, 1, 0, None) == -1
    assert lib.fd_normfac(None, None, 1, 10, None, None) == -1
    assert lib.fd_stitch_chunks(None, 10, None, None, 1, None, 0, None, 10, None) == -1
    assert lib.fd_enhance_chunks(None, None, None, None, None, None, 1.0, 2, 0, None, 1, 30000, None, 0, 0, None) == -1


def test_one_staging_base_and_the_enhance_signatures():
    """FlowModel, ScoreModel and RegressionModel stage their waveforms through ONE base class, and the parameters (names, order, defaults)
    of their `enhance` / `enhance_batch` are the literal ones below."""
    import inspect
    import torch
    import flowdec_amd
    from flowdec_amd import model as M
    classes = (flowdec_amd.FlowModel, flowdec_amd.ScoreModel, flowdec_amd.RegressionModel)
    assert all(c.__bases__ == (M._WaveModel,) for c in classes) and M._WaveModel.__bases__ == (torch.nn.Module,)
    for name in ("_wave_call", "_ragged_call", "_io_entry", "_on_side_stream", "_sync_native", "_preprocess", "_postprocess", "device", "load_state_dict"):
        assert all(name not in vars(c) for c in classes), name                       # owned by the base, overridden nowhere
    assert not hasattr(flowdec_amd.ScoreModel, "enhance_long") and not hasattr(flowdec_amd.RegressionModel, "enhance_long")
    E, VK = inspect.Parameter.empty, "**"
    want = {
        ("FlowModel", "enhance"): [("self", E), ("y", E), ("return_preprocess_info", False), ("N", 50), ("solver", "euler"), ("with_grad", False),
                                   ("sigma_fac", 1.0), ("return_traj", False), ("noise", None), ("generator", None), ("use_graph", True), ("seed", None),
                                   ("step_control", None), ("kwargs", VK)],
        ("FlowModel", "enhance_batch"): [("self", E), ("clips", E), ("N", 50), ("solver", "euler"), ("sigma_fac", 1.0), ("noise", None), ("generator", None),
                                         ("use_graph", True), ("seeds", None), ("step_control", None), ("atol", 0.001), ("rtol", 0.001)],
        ("ScoreModel", "enhance"): [("self", E), ("y", E), ("sampler_type", "pc"), ("predictor", "reverse_diffusion"), ("corrector", "ald"), ("N", 30),
                                    ("corrector_steps", 1), ("snr", 0.5), ("return_preprocess_info", False), ("denoise", True), ("noise", None),
                                    ("generator", None), ("use_graph", True), ("seed", None), ("kwargs", VK)],
        ("ScoreModel", "enhance_batch"): [("self", E), ("clips", E), ("predictor", "reverse_diffusion"), ("corrector", "ald"), ("N", 30), ("corrector_steps", 1),
                                          ("snr", 0.5), ("denoise", True), ("noise", None), ("generator", None), ("seeds", None), ("use_graph", True),
                                          ("kwargs", VK)],
        ("RegressionModel", "enhance"): [("self", E), ("y", E), ("return_preprocess_info", False), ("use_graph", True), ("kwargs", VK)],
        ("RegressionModel", "enhance_batch"): [("self", E), ("clips", E), ("use_graph", True)],
    }
    for c in classes:
        for fn in ("enhance", "enhance_batch"):
            got = [(k, VK if p.kind is p.VAR_KEYWORD else p.default) for k, p in inspect.signature(getattr(c, fn)).parameters.items()]
            assert got == want[c.__name__, fn], (c.__name__, fn, got)
            assert all(p.kind in (p.POSITIONAL_OR_KEYWORD, p.VAR_KEYWORD) for p in inspect.signature(getattr(c, fn)).parameters.values())


def test_cli_argument_errors(tmp_path, capsys):
    from flowdec_amd import enhance_cli
    from test_cli_baselines_cpu import SDE, T_EPS, ckpt_of
    p = enhance_cli.build_parser()
    base = ["--ckpt", "x", "--files", str(tmp_path), "--outdir", str(tmp_path / "o"), "--N", "2"]
    assert p.parse_args(base).chunk_seconds is None
    assert p.parse_args(base + ["--chunk-seconds", "29.7"]).chunk_seconds == 29.7

    def refused(argv, word, model=None):
        with pytest.raises(SystemExit) as e:
            enhance_cli.run(argv, model)
        assert e.value.code == 2 and word in capsys.readouterr().err

    refused(base + ["--chunk-seconds", "10"], "--rng native")                                   # the default --rng torch
    refused(base + ["--chunk-seconds", "10", "--rng", "torch", "--seed", "1"], "--rng native")
    refused(base + ["--chunk-seconds", "0", "--rng", "native"], "positive")
    refused(base + ["--chunk-seconds", "10", "--rng", "native", "--model", "score"], "flow model")
    refused(base + ["--chunk-seconds", "10", "--rng", "native", "--solver", "dopri5"], "fixed-step")
    score = enhance_cli.model_from_checkpoint(ckpt_of("flowdec.model.ScoreModel", SDE, T_EPS))    # the checkpoint names another class
    refused(base + ["--chunk-seconds", "10", "--rng", "native", "--seed", "1"], "flow checkpoint", model=score)
    assert not (tmp_path / "o").exists() or not list((tmp_path / "o").iterdir())


def test_cli_long_file_over_memory_is_skipped(tmp_path, capsys):
    """A long file whose rows do not fit (WorkspaceTooLarge from enhance_long) is skipped with a message, like a file over memory on the
    one-file path: nothing is written, the run goes on and its exit status is 3."""
    import types
    import torch
    from flowdec_amd import enhance_cli

    class Stub:
        sampling_rate = 48000
        feature_extractor = types.SimpleNamespace(_cfg=lambda: {"hop": 384})

        def enhance_long(self, y, **kw):
            self.kw = kw
            raise enhance_cli.WorkspaceTooLarge("the call needs a workspace of 1 byte")

    m, res = Stub(), enhance_cli.RunResult()
    args = types.SimpleNamespace(chunk_seconds=0.6, rtf=False, N=2, solver="euler", seed=3, batch_files=4, precision="bf16")
    job = enhance_cli.FileJob(5, "in.wav", str(tmp_path / "out.wav"), None, True)
    enhance_cli.enhance_file(m, job, args, None, res, 30.0, y=torch.zeros(1, 60000))
    out = capsys.readouterr().out
    assert (res.n_done, res.n_over_precision_limit, res.exit_code) == (0, 1, 3) and not (tmp_path / "out.wav").exists()
    assert "Skipping file: the call needs a workspace" in out and "Long file: 1.2 s in rows of 64 frames, 4 per call" in out
    assert m.kw["rows_per_call"] == 4 and m.kw["row_frames"] == 64 and m.kw["halo_frames"] == 16
