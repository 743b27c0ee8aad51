"""Host-side tests of the validation loss (no GPU): the crop / pad rule of loss_cli against the validation set's formulas, the routing of
a pairs list and the per-pair seeds, the three reductions, and the golden fixture's own consistency."""
import logging
import os

import numpy as np
import pytest
import torch

from conftest import load_golden


# ---- the validation set's crop / pad rule (data/data_module.py:155-171, random_crop=False) --------------------------------------------------
def _rule(n, target):
    """The formulas as written there: -> (start, stop) of the crop, or (pad_left, pad_right)."""
    pad = max(target - n, 0)
    if pad == 0:
        start = int((n - target) / 2)
        return "crop", start, start + target
    return "pad", pad // 2, pad // 2 + (pad % 2)


@pytest.mark.parametrize("n", [100, 101, 107, 93, 94, 1, 250])
def test_crop_or_pad_follows_the_validation_rule(n):
    from flowdec_amd.loss_cli import crop_or_pad_valid
    target = 100
    x = torch.arange(1, n + 1, dtype=torch.float32)
    y = torch.cat([-x, torch.full((5,), 9.0)])          # y is longer: cut to x first
    cx, cy = crop_or_pad_valid(x, y, target)
    assert cx.shape == cy.shape == (target,)
    what, a, b = _rule(n, target)
    if what == "crop":
        assert torch.equal(cx, x[a:b]) and torch.equal(cy, -x[a:b])
    else:
        assert a + b + n == target and b - a == (target - n) % 2
        assert torch.equal(cx[a:a + n], x) and cx[:a].abs().sum() == 0 and cx[a + n:].abs().sum() == 0
        assert torch.equal(cy, -cx)
    if n == target:
        assert torch.equal(cx, x)
    if n == target + 1:
        assert torch.equal(cx, x[:target])              # start = int(0.5) = 0


def test_crop_refuses_a_short_coded_signal():
    from flowdec_amd.loss_cli import crop_or_pad_valid, truncate_pair
    x, y = torch.zeros(50), torch.zeros(49)
    with pytest.raises(ValueError, match="shorter"):
        crop_or_pad_valid(x, y, 40, "p")
    with pytest.raises(ValueError, match="shorter"):
        truncate_pair(x, y, "p")
    a, b = truncate_pair(torch.zeros(50), torch.zeros(60))
    assert a.shape == b.shape == (50,)


# ---- the reductions ------------------------------------------------------------------------------------------------------------------------
def test_reductions_on_hand_made_sums(caplog):
    from flowdec_amd import loss as fd_loss
    sums = np.array([8.0, 2.0, 6.0])
    assert fd_loss.per_clip_values("flow", sums, 4).tolist() == [2.0, 0.5, 1.5]
    assert fd_loss.per_clip_values("regression", sums, [4, 2, 3]).tolist() == [2.0, 1.0, 2.0]
    assert fd_loss.per_clip_values("score", sums, 4).tolist() == [8.0, 2.0, 6.0]
    assert fd_loss.reduce_values("flow", [2.0, 0.5, 1.5]) == pytest.approx(4.0 / 3)
    assert fd_loss.reduce_values("score", sums) == pytest.approx(0.5 * 16.0 / 3)
    assert fd_loss.reduce_values("regression", [2.0, 0.5, 1.5]) == pytest.approx(4.0 / 3)
    # the flow model's NaN rule (model.py:446-467): drop with a warning, give up when all are NaN
    with caplog.at_level(logging.WARNING, logger="flowdec_amd.loss"):
        assert fd_loss.reduce_values("flow", [2.0, float("nan"), 1.0], names=["a", "b", "c"]) == 1.5
    assert "b" in caplog.text and "NaN" in caplog.text
    with pytest.raises(ValueError, match="NaN"):
        fd_loss.reduce_values("flow", [float("nan"), float("nan")])
    # the other two classes propagate a NaN like the reference's plain mean
    assert np.isnan(fd_loss.reduce_values("score", [1.0, float("nan")]))
    assert np.isnan(fd_loss.reduce_values("regression", [1.0, float("nan")]))
    with pytest.raises(ValueError):
        fd_loss.reduce_values("flow", [])
    with pytest.raises(ValueError):
        fd_loss.reduce_values("other", [1.0])


def test_golden_fixture_is_consistent():
    """The stored losses are the stored per-clip values reduced by the three rules (float32 there: 1e-6 relative), and the per-clip
    values are the float64 sums over the F * T_pad = 768 * 64 bins."""
    from flowdec_amd import loss as fd_loss
    g = load_golden("g33_valid_loss.npz")
    n_bins = 768 * 64
    names = [k[:-5] for k in g.files if k.endswith("_loss")]
    assert sorted(names) == ["flow_curve_sx0", "flow_curve_sx01", "flow_scalar_sx0", "flow_scalar_sx01", "regression", "score"]
    for name in names:
        kind = name.split("_")[0]
        per_clip, sums = g[name + "_per_clip"].astype(np.float64), g[name + "_sums"]
        assert per_clip.shape == sums.shape == (2,) and g[name + "_vnorm2"].shape == (2,)
        assert fd_loss.reduce_values(kind, per_clip) == pytest.approx(float(g[name + "_loss"]), rel=1e-6)
        assert fd_loss.per_clip_values(kind, sums, n_bins) == pytest.approx(per_clip, rel=2e-6)
    assert g["x"].shape == g["y"].shape == (2, 1, 12000)
    u = g["u"]
    assert np.array_equal(g["flow_curve_sx01_t"], u) and np.array_equal(g["regression_t"], np.zeros(2, np.float32))
    t_eps = np.float32(g["t_eps"])
    assert np.array_equal(g["score_t"], u * np.float32(1 - t_eps) + t_eps)
    fs = int(g["state_fstride"])
    assert g["state_Xt"].shape == g["state_Ut"].shape == g["state_Y"].shape == (1, 1, 768 // fs, 64)
    assert np.all(g["state_Y"][..., 32:] == 0) and np.all(g["state_X"][..., 32:] == 0)     # 12000 samples: 32 frames, zero tail


# ---- per-pair seeds and bucketing ------------------------------------------------------------------------------------------------------------
def test_pair_seeds():
    from flowdec_amd import loss as fd_loss
    from flowdec_amd.noise import clip_seed
    assert fd_loss.pair_seeds(None, 3) is None
    assert fd_loss.pair_seeds(5, 3) == [clip_seed(5, i) for i in range(3)]
    assert fd_loss.pair_seeds([7, 8, 9], 3) == [7, 8, 9]
    assert fd_loss.pair_seeds(torch.tensor([1, -1]), 2) == [1, -1]
    with pytest.raises(ValueError):
        fd_loss.pair_seeds([1, 2], 3)


def test_batch_buckets_by_padded_frames_and_keeps_list_order(monkeypatch):
    """valid_loss_batch with the native call stubbed: pairs go to the call of their T_pad bucket, at most max_batch per call, pair i carries
    clip_seed(seed, i) wherever it lands, and the results come back in list order."""
    import flowdec_amd
    from flowdec_amd import loss as fd_loss
    from flowdec_amd.noise import clip_seed
    m = flowdec_amd.from_preset("flowdec_75m", precision="bf16", nf=8)
    calls = []

    def fake_native(model, kind, cfg, x_rows, y_rows, lens, seeds, noise, t):
        B, Lrow = y_rows.shape
        Tp = (Lrow + 1) // 384
        calls.append((Tp, list(lens), [int(s) for s in seeds]))
        for b, n in enumerate(lens):
            assert float(x_rows[b, :n].abs().min()) > 0 and float(x_rows[b, n:].abs().sum()) == 0
        sums = torch.tensor([float(y_rows[b, 0]) for b in range(B)], dtype=torch.float64)
        return dict(sums=sums, bad=torch.zeros(B, dtype=torch.int64), normfac=torch.tensor([float(n) for n in lens]),
                    t=torch.tensor([(int(s) % 1000) / 1000.0 for s in seeds]), n_bins=768 * Tp)
    monkeypatch.setattr(fd_loss, "_native", fake_native)
    monkeypatch.setattr(fd_loss, "_require_gpu", lambda model: torch.device("cpu"))
    lengths = [12000, 25000, 9217, 12000, 30000]
    xs = [torch.full((n,), float(i + 1)) for i, n in enumerate(lengths)]
    ys = [torch.full((n,), float(10 * (i + 1))) for i, n in enumerate(lengths)]
    vals, t = m.valid_loss_batch(xs, ys, seeds=3, reduce="none", return_t=True, max_batch=2)
    seeds = [clip_seed(3, i) for i in range(5)]
    two = lambda v: v - (1 << 64) if v >> 63 else v
    assert [(c[0], c[1]) for c in calls] == [(64, [12000, 9217]), (64, [12000]), (128, [25000, 30000])]
    assert [c[2] for c in calls] == [[two(seeds[0]), two(seeds[2])], [two(seeds[3])], [two(seeds[1]), two(seeds[4])]]
    n_bins = np.array([768 * 64, 768 * 128, 768 * 64, 768 * 64, 768 * 128], np.float64)
    assert np.array_equal(vals, np.array([10.0, 20.0, 30.0, 40.0, 50.0]) / n_bins)
    assert m.last_loss_info["normfac"].tolist() == [float(n) for n in lengths]
    assert t.tolist() == pytest.approx([(two(s) % 1000) / 1000.0 for s in seeds])
    with pytest.raises(RuntimeError, match="same shape"):
        m.valid_loss_batch(xs, [y[:-1] for y in ys], seeds=3)
    with pytest.raises(ValueError, match="ambiguous"):
        m.valid_loss_batch(xs, ys, seeds=3, noise=[None] * 5)


# ---- the command line ------------------------------------------------------------------------------------------------------------------------
class _StubModel:
    sampling_rate = 48000

    def __init__(self):
        self.seen = None

    def valid_loss_batch(self, xs, ys, **kw):
        self.seen = dict(xs=xs, ys=ys, **kw)
        n = len(xs)
        return np.arange(1, n + 1, dtype=np.float64), torch.linspace(0.1, 0.9, n)


def test_cli_routes_the_pairs_list(tmp_path):
    from flowdec_amd import loss_cli
    from flowdec_amd.enhance_cli import save_wav
    rng = np.random.default_rng(0)
    lens = [(96000, 96000), (96001, 96010), (40000, 40000), (120000, 120000)]
    lines = []
    for i, (nx, ny) in enumerate(lens):
        fx, fy = tmp_path / f"clean{i}.wav", tmp_path / f"coded{i}.wav"
        chans = 2 if i == 2 else 1
        save_wav(str(fx), torch.from_numpy(0.1 * rng.standard_normal((chans, nx)).astype(np.float32)), 48000)
        save_wav(str(fy), torch.from_numpy(0.1 * rng.standard_normal((1, ny)).astype(np.float32)), 48000)
        lines.append(f"{fx} ---> {fy}")
    pairs = tmp_path / "pairs.txt"
    pairs.write_text("\n".join(lines) + "\n")
    stub = _StubModel()
    csv = tmp_path / "losses.csv"
    import io
    buf = io.StringIO()
    res = loss_cli.run(["--ckpt", "unused", "--pairs-file", str(pairs), "--seed", "5", "--batch", "3", "--out", str(csv)], model=stub, out=buf)
    seen = stub.seen
    assert seen["seeds"] == 5 and seen["max_batch"] == 3 and seen["reduce"] == "none" and seen["return_t"] is True
    assert [tuple(x.shape) for x in seen["xs"]] == [(96000,)] * 4 and [tuple(y.shape) for y in seen["ys"]] == [(96000,)] * 4
    assert float(seen["xs"][2][:28000].abs().sum()) == 0 and float(seen["xs"][2][28000 + 40000:].abs().sum()) == 0   # symmetric pad, mono mean
    assert res.kind == "flow" and res.loss == pytest.approx(2.5) and res.names == [f"coded{i}.wav" for i in range(4)]
    assert buf.getvalue().startswith("valid_loss = 2.5")
    rows = csv.read_text().strip().splitlines()
    assert rows[0] == "name,t,loss" and len(rows) == 5 and rows[1].startswith("coded0.wav,") and rows[4].endswith(",4.0")
    # --no-crop keeps the lengths (y cut to x)
    loss_cli.run(["--ckpt", "unused", "--pairs-file", str(pairs), "--no-crop"], model=stub, out=io.StringIO())
    assert [x.shape[-1] for x in stub.seen["xs"]] == [96000, 96001, 40000, 120000] == [y.shape[-1] for y in stub.seen["ys"]]
    plain = tmp_path / "plain.txt"
    plain.write_text(f"{tmp_path / 'coded0.wav'}\n")
    with pytest.raises(ValueError, match="pair"):
        loss_cli.run(["--ckpt", "unused", "--pairs-file", str(plain)], model=stub, out=io.StringIO())
