"""Streaming for the ScoreDec and regression baselines on the GPU (flowdec_amd/stream.py, stream_cli.py; include/flowdec_hip.h
"Streaming").  The contract of tests/test_hip_stream.py for the two other classes: what a session returns, concatenated, is the class's
long form on the concatenated input (`_WaveModel._enhance_long`, which tests/test_hip_baselines_longform.py reduces to the one-row calls)
bit for bit, however the input was cut and whichever sessions shared its native calls.  Rows of 64 frames, halos of 8, N = 2."""
import numpy as np
import pytest
import torch

from test_hip_baselines import baseline
from test_hip_baselines_longform import CLASSES, GEO, long_form
from test_hip_longform import HALO, N3, N4, RF, STRIDE, W
from test_hip_stream import _late_peak_file

pytestmark = pytest.mark.gpu

PUSHES = (1, 4800, 7919)


def _stream(m, y, seed, normfac, sampler):
    from flowdec_amd.stream import EnhanceStream
    st = EnhanceStream(m, seed=seed, normfac=normfac, **GEO, **sampler)
    outs, pos, i = [], 0, 0
    while pos < len(y):
        k = PUSHES[i % 3]
        outs.append(st.push(y[pos:pos + k]))
        pos, i = pos + k, i + 1
    outs.append(st.flush())
    return torch.cat(outs).cpu(), st.pool


@pytest.mark.parametrize("normfac", ["causal", 0.25])
@pytest.mark.parametrize("kind", list(CLASSES))
def test_stream_equals_the_long_form(kind, normfac):
    m, sampler = baseline(kind, "bf16"), CLASSES[kind]
    y = torch.from_numpy(_late_peak_file(N3, seed=80))
    ref = long_form(m, y, seed=31, normfac=normfac, **sampler)
    assert ref.shape == y.shape and torch.isfinite(ref).all() and ref.abs().max() > 0
    got, pool = _stream(m, y, 31, normfac, sampler)
    assert got.shape == ref.shape and torch.equal(got, ref), float((got - ref).abs().max())
    assert pool.rows_run == pool.native_calls == 3


@pytest.mark.parametrize("kind", list(CLASSES))
def test_pool_sessions_equal_their_long_forms(kind):
    """Three sessions of different lengths, seeds and push schedules in one pool; the regression pool opens its sessions without a seed."""
    from flowdec_amd.stream import StreamPool
    m, sampler = baseline(kind, "bf16"), CLASSES[kind]
    spec = [(W + 1, 101, 4097), (N3, (1 << 63) + 102, 5000), (N4, 103, 4801)]
    ys = [torch.from_numpy(_late_peak_file(n, seed=50 + i)) for i, (n, _, _) in enumerate(spec)]
    pool = StreamPool(m, capacity=4, normfac="causal", **GEO, **sampler)
    sids = [pool.open([seed]) if kind == "score" else pool.open() for _, seed, _ in spec]
    outs = {sid: [] for sid in sids}
    pos, shared = [0, 0, 0], 0
    while any(p < n for p, (n, _, _) in zip(pos, spec)):
        for i, (n, _, block) in enumerate(spec):
            if pos[i] < n:
                k = min(n - pos[i], block)
                pool.push(sids[i], ys[i][pos[i]:pos[i] + k])
                pos[i] += k
        got = pool.step()
        shared += len(got) > 1
        for sid, o in got.items():
            outs[sid].append(o)
    while True:
        got = pool.step()
        if not got:
            break
        for sid, o in got.items():
            outs[sid].append(o)
    for sid in sids:
        outs[sid].append(pool.flush(sid))
    assert shared >= 1, "no native call carried two sessions: the test shows nothing"
    assert pool.rows_run == 2 + 3 + 4 and pool.native_calls < pool.rows_run
    for i, (n, seed, _) in enumerate(spec):
        want = long_form(m, ys[i], seed=[seed], normfac="causal", **sampler)
        assert torch.equal(torch.cat(outs[sids[i]]).cpu(), want), f"session {i}"


@pytest.mark.parametrize("kind", list(CLASSES))
def test_stream_cli_runs_the_class_the_checkpoint_names(kind, tmp_path, capsys):
    from test_cli_baselines_cpu import SDE, T_EPS, ckpt_of
    from flowdec_amd import enhance_cli, stream_cli
    ckpt = ckpt_of("flowdec.model.ScoreModel", SDE, T_EPS) if kind == "score" else ckpt_of("flowdec.model.RegressionModel")
    torch.save(ckpt, tmp_path / "m.ckpt")
    n = STRIDE + W + 123
    y = _late_peak_file(n, seed=70)
    y.astype("<f4").tofile(tmp_path / "in.raw")
    flags = ["--predictor", "euler_maruyama", "--corrector", "ald", "--corrector-steps", "2", "--snr", "0.4"] if kind == "score" else []
    written = stream_cli.run(["--ckpt", str(tmp_path / "m.ckpt"), "--N", "2", "--seed", "7", "--row-frames", str(RF), "--halo-frames", str(HALO),
                              "--normfac", "causal", "--format", "f32le", "--in", str(tmp_path / "in.raw"), "--out", str(tmp_path / "out.raw"),
                              "--block-samples", "4801"] + flags)
    err = capsys.readouterr().err
    m = enhance_cli.load_from_checkpoint(str(tmp_path / "m.ckpt"), map_location="cuda:0")
    assert type(m).__name__ == {"score": "ScoreModel", "regression": "RegressionModel"}[kind]
    sampler = dict(N=2, predictor="euler_maruyama", corrector="ald", corrector_steps=2, snr=0.4) if kind == "score" else {}
    want = long_form(m, torch.from_numpy(y), seed=7, normfac="causal", **sampler)
    assert written == n and torch.isfinite(want).all() and want.abs().max() > 0
    assert (tmp_path / "out.raw").read_bytes() == stream_cli.encode(want, "f32le")
    assert ("are ignored" in err) == (kind == "regression")


def test_stream_cli_codes_with_a_regression_model(tmp_path):
    """`--codes` through a small random NDAC == the PCM path fed the one-shot decode, byte for byte, with a baseline behind the decoder."""
    from flowdec_amd import stream_cli
    from flowdec_amd.ndac import DAC
    from test_hip_ndac_stream import NDAC75_LIKE, codes_of
    from test_ndac_cpu import scaled_sd
    m = baseline("regression", "bf16")
    cfg, nq, T = NDAC75_LIKE, 4, 45
    sd = scaled_sd(cfg, 5, 0.6)
    torch.save({"state_dict": {k: torch.from_numpy(v) for k, v in sd.items()},
                "metadata": {"kwargs": dict(cfg, encoder_rates=list(cfg["encoder_rates"]), decoder_rates=list(cfg["decoder_rates"]))}}, tmp_path / "weights.pth")
    dac = DAC.load(str(tmp_path / "weights.pth")).cuda()
    assert dac.sample_rate == m.sampling_rate
    codes = codes_of(dac, nq, T, 9)
    codes.numpy().T.astype("<i2").tofile(tmp_path / "codes.raw")
    dac.decode(dac.quantizer.from_codes(codes[None].cuda())[0])[0, 0].cpu().numpy().astype("<f4").tofile(tmp_path / "pcm.raw")
    common = ["--ckpt", "unused", "--N", "2", "--seed", "7", "--row-frames", "64", "--halo-frames", "16", "--normfac", "causal", "--format", "f32le"]
    n_pcm = stream_cli.run(common + ["--in", str(tmp_path / "pcm.raw"), "--out", str(tmp_path / "a.raw"), "--block-samples", "4801"], model=m)
    n_codes = stream_cli.run(common + ["--codes", "--codec", str(tmp_path / "weights.pth"), "--n-quantizers", str(nq), "--decode-block-frames", "3",
                                       "--in", str(tmp_path / "codes.raw"), "--out", str(tmp_path / "b.raw"), "--block-samples", "37"], model=m)
    a, b = (tmp_path / "a.raw").read_bytes(), (tmp_path / "b.raw").read_bytes()
    assert n_pcm == n_codes == T * dac.hop_length and len(a) == 4 * n_pcm and a == b
    out = np.frombuffer(a, dtype="<f4")
    assert np.isfinite(out).all() and np.abs(out).max() > 0
