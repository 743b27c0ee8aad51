"""The device resampler's host side (include/flowdec_hip.h "Resampling"; flowdec_amd/resample.py): nothing here needs a GPU.

The NumPy restatement of the kernel's arithmetic (tests/resample_oracle.py) against the shipped host resampler within a derived bound;
the 64-bit length rule; the streaming planner's invariants; the argument checks of fd_resample_plan_create; the command lines' flags."""
import ctypes as C

import numpy as np
import pytest
import torch

import resample_oracle as RO

# (orig, new, lowpass_filter_width)
PAIRS = [(44100, 48000, 64), (44100, 48000, 256), (16000, 48000, 64), (48000, 16000, 64), (48000, 44100, 64)]


def _lib():
    import __graft_entry__ as g
    g.build()
    from flowdec_amd import _lib
    return _lib.load()


def bound(bank, o, n, width, x, y):
    """Per output: any-order float32 accumulation of K products, each rounded (K + 1 roundings of magnitude <= sum |h x|), against the
    exact sum rounded once: (K + 1) 2^-24 sum_k |h x| + 2^-24 |y|."""
    K = 2 * width + o
    return (K + 1) * 2.0 ** -24 * RO.abs_sum(bank, o, n, width, x) + 2.0 ** -24 * np.abs(y.astype(np.float64))


@pytest.mark.parametrize("orig,new,lpw", PAIRS)
def test_restatement_against_host_resampler_within_derived_bound(orig, new, lpw):
    from flowdec_amd.enhance_cli import resample, sinc_resample_kernel
    bank, width, o, n = sinc_resample_kernel(orig, new, lpw)
    x = np.random.default_rng(orig + new + lpw).standard_normal(3000).astype(np.float32)
    want = resample(torch.from_numpy(x)[None], orig, new, lowpass_filter_width=lpw)[0].numpy()
    got = RO.resample(bank, o, n, width, x)
    assert got.shape == want.shape == (RO.out_length(len(x), o, n),)
    err, b = np.abs(got.astype(np.float64) - want.astype(np.float64)), bound(bank, o, n, width, x, got)
    print(f"{orig}->{new} lpw {lpw}: max |diff| / bound = {float((err / b).max()):.3f}")
    assert np.all(err <= b)


def test_restatement_spans_equal_the_one_shot():
    """An output range computed from a window of the recording, with the total unknown or known, has the one-shot's bits."""
    from flowdec_amd.enhance_cli import sinc_resample_kernel
    bank, width, o, n = sinc_resample_kernel(44100, 48000)
    x = np.random.default_rng(3).standard_normal(1500).astype(np.float32)
    full = RO.resample(bank, o, n, width, x)
    m0, count = 3 * n + 7, 4 * n + 1                      # periods 3..7: samples [3 o - width, 7 o + width + o - 1]
    lo, hi = max(0, 3 * o - width), 7 * o + width + o
    assert np.array_equal(RO.resample(bank, o, n, width, x[lo:hi], x0=lo, total=-1, m0=m0, count=count), full[m0:m0 + count])
    tail0 = len(full) - 200
    lo = max(0, (tail0 // n) * o - width)
    assert np.array_equal(RO.resample(bank, o, n, width, x[lo:], x0=lo, total=len(x), m0=tail0), full[tail0:])
    with pytest.raises(AssertionError):
        RO.resample(bank, o, n, width, x[10:600], x0=10, total=-1, m0=0, count=1)      # period 0 reads the samples 0..9 too


def test_out_length_against_resampled_length():
    from flowdec_amd.enhance_cli import resampled_length
    from flowdec_amd.resample import Resampler, rate_ratio
    lib = _lib()
    for orig, new in [(44100, 48000), (48000, 44100), (16000, 48000), (48000, 16000), (8000, 48000), (22050, 48000)]:
        o, n, _ = rate_ratio(orig, new)
        lengths = [0, 1, 2, max(o - 1, 0), o, o + 1, n, 4410, 30000, 2 ** 31 - 1, 2 ** 31, 2 ** 31 + 1, 2 ** 31 + o - 1, 2 ** 33 + 12345]
        for length in lengths:
            got = lib.fd_resample_out_length(length, o, n)
            assert got == resampled_length(length, orig, new) == -(-n * length // o), (orig, new, length)
    assert lib.fd_resample_out_length(2 ** 46, 1, 2 ** 16) == 2 ** 62                  # no 32-bit intermediate, no n * L overflow below 2^63
    assert lib.fd_resample_out_length(2 ** 46 + 1, 2 ** 24 - 1, 2 ** 24) == -(-(2 ** 24) * (2 ** 46 + 1) // (2 ** 24 - 1))   # n * L is beyond 2^63 here
    assert lib.fd_resample_out_length(-1, 1, 1) == -1 and lib.fd_resample_out_length(5, 0, 1) == -1
    r = Resampler(48000, 48000, device="cpu")                                        # equal rates need neither a plan nor a GPU
    assert r.identity and r.out_length(777) == 777


@pytest.mark.parametrize("o,n,width", [(147, 160, 65), (160, 147, 72), (1, 3, 65), (3, 1, 194), (5, 7, 0)])
def test_planner_random_cuts(o, n, width):
    from flowdec_amd.resample import ResamplePlanner
    rng = np.random.default_rng(o * 1000 + n)
    for trial in range(6):
        total = int(rng.integers(0, 12 * o + 3 * width + 2))
        cuts, left = [], total
        while left:
            k = int(rng.choice([0, 1, 1, int(rng.integers(1, 2 * o + 2)), int(rng.integers(1, total + 1))]))
            k = min(k, left)
            cuts.append(k)
            left -= k
        cuts += [0] * (trial % 2)
        p = ResamplePlanner(o, n, width)
        assert p.delay_samples == width + o
        got, received = 0, 0
        for k in cuts + [None]:
            rel = p.push(k) if k is not None else p.flush()
            received += k or 0
            assert rel.m0 == got and rel.count >= 0                                       # in order, no gap, no overlap
            got += rel.count
            if k is not None:
                # nothing released needs a sample not yet received; the next output does (the range is maximal)
                assert got == 0 or ((got - 1) // n) * o + width + o - 1 < received
                assert (got // n) * o + width + o - 1 >= received
            # the retention index: the next output's first tap, never past a sample that is still needed
            assert 0 <= rel.retain_from <= max(0, (got // n) * o - width) and rel.retain_from == p.retain_from
        assert got == -(-n * total // o)
        with pytest.raises(RuntimeError):
            p.push(1)


def test_plan_create_refuses_bad_arguments_without_a_gpu():
    from flowdec_amd import _lib as L
    lib = _lib()
    bank = np.zeros(8, dtype=np.float32)
    bp = bank.ctypes.data_as(C.c_void_p)
    plan = C.c_void_p()
    for args in [(None, 147, 160, 65), (bp, 0, 160, 65), (bp, 147, 0, 65), (bp, 147, 160, -1), (bp, -3, 1, 1),
                 (bp, 47999, 48000, 65),                     # 47999 -> 48000 at lowpass_filter_width 64: 2.3 * 10^9 coefficients, 9 GB
                 (bp, 2 ** 24, 2, 0),                        # n K = 2^25
                 (bp, 1, 2 ** 24 + 1, 0)]:
        assert lib.fd_resample_plan_create(*args, C.byref(plan)) == -1, args
        assert not plan.value and lib.fd_last_error()
    assert lib.fd_resample_plan_create(bp, 1, 1, 0, None) == -1
    lib.fd_resample_plan_destroy(None)
    from flowdec_amd.resample import BANK_CAP, Resampler, bank_fits, rate_ratio
    assert rate_ratio(47999, 48000) == (47999, 48000, 65) and BANK_CAP == 2 ** 24
    assert not bank_fits(47999, 48000) and bank_fits(44100, 48000, 256) and bank_fits(48000, 48000)
    with pytest.raises(ValueError, match="47999 -> 48000"):
        Resampler(47999, 48000, device="cuda")              # refused before anything touches a device
    with pytest.raises(RuntimeError, match="fd_resample_plan_create|flowdec_hip error"):
        L.check(lib.fd_resample_plan_create(bp, 0, 1, 1, C.byref(plan)))


def test_parsers():
    from flowdec_amd import enhance_cli, estimate_cli, eval_cli, stream_cli
    base = ["--ckpt", "c", "--files", "f", "--outdir", "o", "--N", "1"]
    assert enhance_cli.build_parser().parse_args(base).resample == "host"
    assert enhance_cli.build_parser().parse_args(base + ["--resample", "device"]).resample == "device"
    ev = ["--triples", "t", "--out", "o"]
    assert eval_cli.build_parser().parse_args(ev).resample == "host" and eval_cli.build_parser().parse_args(ev + ["--resample", "device"]).resample == "device"
    es = ["--pairs-file", "p", "--alpha", "0.3", "--nfft", "1534", "--hop", "384"]
    assert estimate_cli.build_parser().parse_args(es).resample == "host"
    assert estimate_cli.build_parser().parse_args(es + ["--resample", "device"]).resample == "device"
    for parser, argv in ((enhance_cli.build_parser(), base), (eval_cli.build_parser(), ev), (estimate_cli.build_parser(), es)):
        with pytest.raises(SystemExit):
            parser.parse_args(argv + ["--resample", "gpu"])
        assert "float32 rounding" in " ".join(parser.format_help().split())
    st = ["--ckpt", "c", "--N", "2", "--seed", "1", "--normfac", "causal", "--format", "s16le"]
    a = stream_cli.parse_args(st)
    assert a.in_rate is None and a.out_rate is None
    a = stream_cli.parse_args(st + ["--in-rate", "44100", "--out-rate", "16000"])
    assert (a.in_rate, a.out_rate) == (44100, 16000)
    with pytest.raises(SystemExit):
        stream_cli.parse_args(st + ["--in-rate", "0"])


def test_load_mono_host_is_the_default(tmp_path):
    """load_mono(path, sr) and resample='host' are today's host path; an unknown mode is refused."""
    from flowdec_amd import enhance_cli, eval_cli
    x = (0.1 * np.random.default_rng(0).standard_normal(2000)).astype(np.float32)
    enhance_cli.save_wav(str(tmp_path / "a.wav"), torch.from_numpy(x), 16000)
    want = enhance_cli.resample(torch.from_numpy(x)[None], 16000, 48000, lowpass_filter_width=256)[0]
    assert torch.equal(eval_cli.load_mono(str(tmp_path / "a.wav"), 48000), want)
    assert torch.equal(eval_cli.load_mono(str(tmp_path / "a.wav"), 48000, resample="host"), want)
    with pytest.raises(ValueError):
        eval_cli.load_mono(str(tmp_path / "a.wav"), 48000, resample="gpu")


def test_pair_over_the_bank_cap_falls_back_to_the_host_with_one_line(tmp_path, capsys, monkeypatch):
    """47999 -> 48000 Hz asks for a 9 GB bank: --resample device then takes the host path (stubbed here: only the routing is under test)
    and says so in one line; no GPU is touched."""
    from types import SimpleNamespace
    from flowdec_amd import audio, enhance_cli, eval_cli
    calls = []

    def host(y, sr, target, lowpass_filter_width=64, rolloff=0.99):
        calls.append((sr, target, lowpass_filter_width))
        return y + 1

    monkeypatch.setattr(audio, "resample", host)      # the one router (audio.resample_to) serves both command lines
    x = torch.from_numpy((0.1 * np.random.default_rng(5).standard_normal((1, 300))).astype(np.float32))
    capsys.readouterr()
    got = enhance_cli.resample_for_model(x, 47999, SimpleNamespace(sampling_rate=48000, device=torch.device("cuda:0")), "device")
    lines = [l for l in capsys.readouterr().out.splitlines() if "47999" in l]
    assert len(lines) == 1 and "host" in lines[0] and torch.equal(got, x + 1) and calls == [(47999, 48000, 64)]
    enhance_cli.save_wav(str(tmp_path / "a.wav"), x, 47999)
    got = eval_cli.load_mono(str(tmp_path / "a.wav"), 48000, resample="device")
    lines = [l for l in capsys.readouterr().out.splitlines() if "47999" in l]
    assert len(lines) == 1 and "host" in lines[0] and torch.equal(got, x[0] + 1) and calls[1:] == [(47999, 48000, 256)]


def test_gpus_worker_command_carries_resample(tmp_path, monkeypatch):
    """A --gpus N worker is a fresh process of the module: its command line must carry --resample."""
    from flowdec_amd import enhance_cli
    (tmp_path / "in").mkdir()
    seen = []

    class Started(Exception):
        pass

    def popen(cmd, **kw):
        seen.append(list(cmd))
        raise Started()

    monkeypatch.setattr(enhance_cli.subprocess, "Popen", popen)
    argv = ["--ckpt", str(tmp_path / "none.ckpt"), "--files", str(tmp_path / "in"), "--outdir", str(tmp_path / "out"), "--N", "1",
            "--gpus", "2", "--share-gpu", "--resample", "device"]
    with pytest.raises(Started):
        enhance_cli.run(argv)
    cmd = seen[0]
    assert cmd[cmd.index("--resample") + 1] == "device" and "--worker-rank" in cmd
    assert enhance_cli.build_parser().parse_args(cmd[cmd.index("flowdec_amd.enhance_cli") + 1:]).resample == "device"
