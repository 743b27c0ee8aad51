"""The device resampler on the GPU (include/flowdec_hip.h "Resampling"; csrc/resample.hip; flowdec_amd/resample.py).

Every comparison against the NumPy restatement (tests/resample_oracle.py) and between launch shapes is BIT FOR BIT: the contract fixes
the order of every sum.  The host resampler `enhance_cli.resample` sums in float32 in an unspecified order, so against it the derived
bound of tests/test_resample_cpu.py applies.  Model and geometry of the streaming tests: tests/test_hip_stream.py."""
import numpy as np
import pytest
import torch

import resample_oracle as RO
from test_hip_longform import HALO, N3, RF, _file, _flow
from test_resample_cpu import bound

pytestmark = pytest.mark.gpu

KW = dict(N=2, solver="euler", row_frames=RF, halo_frames=HALO)
# (orig, new, lowpass_filter_width): 44.1 -> 48 k is n = 160, o = 147, K = 277 / 665; 16 -> 48 k o = 1; 48 -> 16 k n = 1.
# 48000 -> 1000 (o = 48, n = 1, K = 6256) is the pair whose input window does not fit the LDS budget: the kernel's global-memory path
PAIRS = [(44100, 48000, 64), (44100, 48000, 256), (16000, 48000, 64), (48000, 16000, 64), (48000, 44100, 64), (8000, 48000, 64), (48000, 1000, 64)]
_banks = {}


def _bank(orig, new, lpw=64):
    from flowdec_amd.enhance_cli import sinc_resample_kernel
    if (orig, new, lpw) not in _banks:
        _banks[orig, new, lpw] = sinc_resample_kernel(orig, new, lpw)
    return _banks[orig, new, lpw]


def _resampler(orig, new, lpw=64):
    from flowdec_amd.resample import get_resampler
    return get_resampler(orig, new, lpw, device="cuda:0")


def _signal(n, seed):
    return np.random.default_rng(seed).standard_normal(n).astype(np.float32)


def _oracle(orig, new, lpw, x, **kw):
    bank, width, o, n = _bank(orig, new, lpw)
    return RO.resample(bank, o, n, width, x, **kw)


# ---- 1. one shot ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("orig,new,lpw", PAIRS)
def test_one_shot_bit_for_bit_against_the_restatement(orig, new, lpw):
    from flowdec_amd.enhance_cli import resample
    bank, width, o, n = _bank(orig, new, lpw)
    r = _resampler(orig, new, lpw)
    assert (r.o, r.n, r.width, r.K) == (o, n, width, 2 * width + o)
    lengths = sorted({L for L in (1, 2, o - 1, o, o + 1, width, 2 * width + o, 3 * o, 4410, 30000) if L >= 1})
    assert any(n * L % o == 0 for L in lengths)
    for L in lengths:
        x = _signal(L, seed=L)
        got = r(torch.from_numpy(x).cuda()).cpu().numpy()
        want = _oracle(orig, new, lpw, x)
        assert got.shape == (-(-n * L // o),) == want.shape == (r.out_length(L),)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (orig, new, lpw, L, int((got != want).sum()))
        if L in (4410, 30000):
            host = resample(torch.from_numpy(x)[None], orig, new, lowpass_filter_width=lpw)[0].numpy()
            err, b = np.abs(got.astype(np.float64) - host.astype(np.float64)), bound(bank, o, n, width, x, got)
            print(f"{orig}->{new} lpw {lpw} L {L}: max |device - host| / bound = {float((err / b).max()):.3f}")
            assert np.all(err <= b)
    assert r.out_length(1) == -(-n // o)


def test_one_shot_shapes_equal_rates_and_refusals():
    from flowdec_amd.resample import Resampler, resample_device
    r = _resampler(44100, 48000)
    x = torch.from_numpy(_signal(3 * 2 * 1000, seed=9)).cuda().reshape(3, 2, 1000)
    y = r(x)
    assert y.shape == (3, 2, r.out_length(1000))
    for a in range(3):
        for b in range(2):
            assert torch.equal(y[a, b], r(x[a, b].clone()))                          # a row's bits do not depend on the batch
    assert torch.equal(resample_device(x, 44100, 48000), y)
    assert torch.equal(resample_device(x, 88200, 96000), y)                          # the ratio decides, the plan is shared
    assert resample_device(x, 48000, 48000) is x and Resampler(48000, 48000, device="cuda:0")(x) is x
    assert r(torch.empty(0, device="cuda")).shape == (0,)
    with pytest.raises(RuntimeError):
        r(x.cpu())
    with pytest.raises(TypeError):
        r(x.double())
    with pytest.raises(ValueError, match="47999 -> 48000"):
        resample_device(x, 47999, 48000)


# ---- 2. ragged batch -----------------------------------------------------------------------------------------------------------------
def _ragged(r, clips, L, L_out):
    """fd_resample on rows of stride L -> (rc, y [B][L_out], prefilled with NaN)."""
    from flowdec_amd import _lib as Lb
    x = torch.full((len(clips), L), float("nan"), device="cuda")                     # behind a clip: never read
    for b, c in enumerate(clips):
        x[b, :len(c)] = torch.from_numpy(c)
    lens = torch.tensor([len(c) for c in clips], dtype=torch.int32, device="cuda")
    y = torch.full((len(clips), L_out), float("nan"), device="cuda")
    rc = Lb.load().fd_resample(r._plan, Lb.ptr(x), Lb.ptr(lens), len(clips), L, Lb.ptr(y), L_out, Lb.stream())
    torch.cuda.synchronize()
    return rc, y.cpu().numpy()


def test_ragged_batch():
    r = _resampler(44100, 48000)
    lens = [1, 146, 147, 4410, 30000]
    clips = [_signal(L, seed=100 + L) for L in lens]
    alone = [r(torch.from_numpy(c).cuda()).cpu().numpy() for c in clips]
    L_out = r.out_length(30000) + 37
    for order in (list(range(5)), [3, 0, 4, 2, 1]):
        rc, y = _ragged(r, [clips[i] for i in order], 30000, L_out)
        assert rc == 0
        for b, i in enumerate(order):
            M = r.out_length(lens[i])
            assert np.array_equal(y[b, :M].view(np.uint32), alone[i].view(np.uint32)), (order, b)
            assert np.array_equal(y[b, M:].view(np.uint32), np.zeros(L_out - M, np.uint32)), (order, b)     # +0.0, no NaN leaked in
    for got, want in zip(r.batch([torch.from_numpy(c).cuda() for c in clips]), alone):
        assert np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32))
    rc, y = _ragged(r, clips, 30000, r.out_length(30000) - 1)
    assert rc == -1 and np.isnan(y).all()                                            # FD_EINVAL, nothing launched


# ---- 3. spans ------------------------------------------------------------------------------------------------------------------------
def test_span_addressing_beyond_32_bits():
    """Shifting the input by c o samples shifts the outputs by c n with the same phases: the span at x0 = c o > 2^33 equals the span at 0."""
    r = _resampler(44100, 48000)
    o, n, width = r.o, r.n, r.width
    x = _signal(3000, seed=5)
    xd = torch.from_numpy(x).cuda()
    c = 2 ** 33 // o + 1
    assert c * o > 2 ** 33 and c * n > 2 ** 33
    for rr, count in ((n, 17 * n), (n + 53, 16 * n + 7), (3 * n - 1, 2)):            # from period 1 on: no tap below sample 0
        assert (rr // n) * o - width >= 0 and ((rr + count - 1) // n) * o + width + o - 1 < len(x)
        base = r.span(xd, 0, -1, rr, count).cpu().numpy()
        far = r.span(xd, c * o, -1, c * n + rr, count).cpu().numpy()
        assert np.array_equal(base.view(np.uint32), far.view(np.uint32)), (rr, count)
        assert np.array_equal(base.view(np.uint32), _oracle(44100, 48000, 64, x, total=-1, m0=rr, count=count).view(np.uint32))
    # a known total far out: the last outputs of a recording that ends inside the buffer
    total = c * o + 2500
    M = RO.out_length(total, o, n)
    m0 = c * n + 10 * n
    far = r.span(xd[:2500], c * o, total, m0, M - m0).cpu().numpy()
    near = r.span(xd[:2500], 0, 2500, 10 * n, RO.out_length(2500, o, n) - 10 * n).cpu().numpy()
    assert len(far) == len(near) and np.array_equal(far.view(np.uint32), near.view(np.uint32))


def test_refused_spans():
    from flowdec_amd import _lib as Lb
    lib = Lb.load()
    r = _resampler(44100, 48000)
    o, n, width = r.o, r.n, r.width
    x = torch.zeros(1000, device="cuda")
    y = torch.full((4 * n,), float("nan"), device="cuda")

    def span(x0, nx, total, m0, count):
        return lib.fd_resample_span(r._plan, Lb.ptr(x), x0, nx, total, m0, count, Lb.ptr(y), Lb.stream())

    assert span(100, 900, -1, 0, 1) == -1                         # period 0 reads the samples 0..99
    assert span(0, 1000, -1, 5 * n, 2 * n) == -1                  # period 6 reads up to 6 o + width + o - 1 = 1093
    assert span(0, 1000, 2000, 5 * n, 2 * n) == -1                # ... which a total of 2000 does not excuse
    assert span(0, 1000, 1000, 0, RO.out_length(1000, o, n) + 1) == -1      # beyond the recording's last output
    assert span(-1, 1000, -1, 0, 1) == -1 and span(0, 1000, -2, 0, 1) == -1 and span(0, 1000, -1, -1, 1) == -1
    assert span(0, 1000, -1, 0, 0) == 0                           # nothing to do
    torch.cuda.synchronize()
    assert torch.isnan(y).all()                                   # a refused call launches nothing
    assert span(0, 1000, 1000, 5 * n, RO.out_length(1000, o, n) - 5 * n) == 0      # the recording ends at 1000: the taps beyond are not read
    assert span(0, 1000, -1, 4 * n, n) == 0                       # 4 o + width + o - 1 = 799


# ---- 4. the stream -------------------------------------------------------------------------------------------------------------------
STREAM_L = 12000
_stream_ref = {}


def _stream_case():
    if not _stream_ref:
        x = np.clip(0.3 * _signal(STREAM_L, seed=77), -0.99, 0.99).astype(np.float32)
        _stream_ref["x"] = x
        _stream_ref["y"] = _resampler(44100, 48000)(torch.from_numpy(x).cuda()).cpu()
    return _stream_ref["x"], _stream_ref["y"]


def _run_stream(blocks, r):
    """Push every block, flush -> the concatenated output; after each push the samples returned so far are what the planner says."""
    from flowdec_amd.resample import ResamplePlanner, ResampleStream
    st, p = ResampleStream(r), ResamplePlanner(r.o, r.n, r.width)
    assert st.delay_samples == r.width + r.o
    outs, got = [], 0
    for blk in blocks:
        outs.append(st.push(blk))
        rel = p.push(int(torch.as_tensor(blk).numel()))
        got += outs[-1].numel()
        assert outs[-1].is_cuda and outs[-1].dtype == torch.float32 and got == rel.m0 + rel.count
    outs.append(st.flush())
    return torch.cat(outs).cpu()


def _cut(x, sizes):
    out, pos = [], 0
    for k in sizes:
        out.append(x[pos:pos + k])
        pos += k
    out.append(x[pos:])
    return out


def test_stream_equals_one_shot_however_it_is_cut():
    x, want = _stream_case()
    r = _resampler(44100, 48000)
    xt = torch.from_numpy(x)
    rng = np.random.default_rng(8)
    cuts = [[1, 1, 146, 147, 148, 277, 5000],
            list(rng.integers(0, 900, 40)), list(rng.integers(0, 3, 50)) + list(rng.integers(100, 4000, 6)),
            [],                                                          # one push of everything
            [STREAM_L]]                                                  # everything, then an empty push before the flush
    for sizes in cuts:
        got = _run_stream(_cut(xt, [int(k) for k in sizes]), r)
        assert torch.equal(got, want), sizes
    dev = _run_stream([b.cuda() for b in _cut(xt, cuts[0])], r)          # device blocks
    mixed = _run_stream([b.cuda() if i % 2 else b.numpy() for i, b in enumerate(_cut(xt, cuts[0]))], r)
    assert torch.equal(dev, want) and torch.equal(mixed, want)
    # a caller may reuse its buffer after push
    from flowdec_amd.resample import ResampleStream
    st, buf, outs = ResampleStream(r), torch.empty(1000, device="cuda"), []
    for pos in range(0, STREAM_L, 1000):
        buf.copy_(xt[pos:pos + 1000])
        outs.append(st.push(buf))
        buf.fill_(float("nan"))
    outs.append(st.flush())
    assert torch.equal(torch.cat(outs).cpu(), want)
    # nothing pushed at all; and other ratios through the same code
    assert _run_stream([], r).numel() == 0
    for orig, new in ((48000, 16000), (16000, 48000), (48000, 44100)):
        r2 = _resampler(orig, new)
        assert torch.equal(_run_stream(_cut(xt, [1, 2, 3, 500, 0, 4000]), r2), r2(xt.cuda()).cpu()), (orig, new)


def test_stream_int16_pushes_equal_float_pushes():
    x, _ = _stream_case()
    r = _resampler(44100, 48000)
    pcm = np.clip(np.rint(x * 32768), -32768, 32767).astype(np.int16)
    pcm[10], pcm[11] = -32768, 32767
    xf = torch.from_numpy(pcm.astype(np.float32) / np.float32(32768))    # exact
    want = r(xf.cuda()).cpu()
    sizes = [1, 1, 146, 147, 148, 277, 5000]
    assert torch.equal(_run_stream(_cut(torch.from_numpy(pcm), sizes), r), want)
    assert torch.equal(_run_stream(_cut(torch.from_numpy(pcm).cuda(), sizes), r), want)
    assert torch.equal(_run_stream(_cut(xf, sizes), r), want)
    from flowdec_amd.resample import ResampleStream
    with pytest.raises(TypeError):
        ResampleStream(r).push(torch.zeros(4, dtype=torch.float64))


# ---- 5. EnhanceStream with rates -----------------------------------------------------------------------------------------------------
def _stream_enhance(m, y, sizes, **kw):
    from flowdec_amd.stream import EnhanceStream
    st = EnhanceStream(m, seed=5, normfac="causal", **dict(KW, **kw))
    outs = [st.push(b) for b in _cut(y, sizes)] + [st.flush()]
    return torch.cat(outs).cpu(), st


def test_enhance_stream_with_rates():
    from flowdec_amd.resample import resample_device
    m = _flow("bf16")
    n_in = -(-N3 * 147 // 160)
    y = torch.from_numpy(_file(n_in, seed=31))
    y48 = resample_device(y.cuda(), 44100, 48000)
    assert 0 <= y48.numel() - N3 <= 2
    want = m.enhance_long(y48, seed=5, normfac="causal", **KW)
    assert torch.isfinite(want).all() and want.abs().max() > 0
    sizes = [1, 4409, 20000, 0, 7001]
    got, st = _stream_enhance(m, y, sizes, in_rate=44100)
    assert torch.equal(got, want.cpu())
    assert st.delays == (65 + 147, st.pool.delay_samples, 0) and st.delay_samples == st.pool.delay_samples
    got, st = _stream_enhance(m, y, sizes, in_rate=44100, out_rate=44100)
    assert torch.equal(got, resample_device(want, 48000, 44100).cpu())
    assert st.delays == (65 + 147, st.pool.delay_samples, 71 + 160)
    # no rates, and the model's own rate: today's stream
    y_model = y48.cpu()
    plain = m.enhance_long(y_model, seed=5, normfac="causal", **KW)
    assert torch.equal(plain, want.cpu())
    for kw in ({}, dict(in_rate=None, out_rate=None), dict(in_rate=48000, out_rate=48000)):
        got, st = _stream_enhance(m, y_model, sizes, **kw)
        assert torch.equal(got, plain) and st.delays == (0, st.pool.delay_samples, 0), kw


def test_stream_cli_in_rate_reproduces_the_api(tmp_path):
    from test_cli import synthetic_ckpt
    from flowdec_amd import enhance_cli, stream_cli
    from flowdec_amd.resample import resample_device
    torch.save(synthetic_ckpt(), tmp_path / "m.ckpt")
    n_in = -(-N3 * 147 // 160)
    pcm = np.clip(np.rint(_file(n_in, seed=32) * 32768), -32768, 32767).astype("<i2")
    pcm.tofile(tmp_path / "in.raw")
    common = ["--ckpt", str(tmp_path / "m.ckpt"), "--N", "2", "--solver", "euler", "--seed", "7", "--row-frames", str(RF), "--halo-frames", str(HALO),
              "--normfac", "causal", "--format", "s16le", "--in", str(tmp_path / "in.raw"), "--block-samples", "4801"]
    written = stream_cli.run(common + ["--out", str(tmp_path / "out.raw"), "--in-rate", "44100"])
    m = enhance_cli.load_from_checkpoint(str(tmp_path / "m.ckpt"), map_location="cuda:0", model="flow")
    y = torch.from_numpy(pcm.astype(np.float32) / np.float32(32768)).cuda()
    want = m.enhance_long(resample_device(y, 44100, 48000), seed=7, normfac="causal", **KW)
    assert written == want.numel() == -(-160 * n_in // 147)
    assert (tmp_path / "out.raw").read_bytes() == stream_cli.encode(want, "s16le")
    written = stream_cli.run(common + ["--out", str(tmp_path / "out2.raw"), "--in-rate", "44100", "--out-rate", "44100"])
    want2 = resample_device(want, 48000, 44100)
    assert written == want2.numel() and (tmp_path / "out2.raw").read_bytes() == stream_cli.encode(want2, "s16le")


# ---- 6. the corpus command lines -----------------------------------------------------------------------------------------------------
def test_enhance_cli_resample_device(tmp_path):
    from test_cli import synthetic_ckpt
    from flowdec_amd import enhance_cli
    from flowdec_amd.resample import resample_device
    torch.save(synthetic_ckpt(), tmp_path / "m.ckpt")
    ind = tmp_path / "in"
    ind.mkdir()
    rng = np.random.default_rng(4)
    spec = [("a", 12000, 16000), ("b", 30000, 44100), ("c", 30000, 48000)]
    files = {}
    for name, n, sr in spec:
        files[name] = torch.from_numpy((0.1 * rng.standard_normal((1, n))).astype(np.float32))
        enhance_cli.save_wav(str(ind / f"{name}.wav"), files[name], sr)
    m = enhance_cli.load_from_checkpoint(str(tmp_path / "m.ckpt"), map_location="cuda:0")
    common = ["--ckpt", str(tmp_path / "m.ckpt"), "--files", str(ind), "--N", "2", "--solver", "euler", "--seed", "11", "--rng", "native"]
    outs = {}
    for mode, extra in (("default", []), ("host", ["--resample", "host"]), ("device", ["--resample", "device"]), ("device1", ["--resample", "device", "--batch-files", "1"])):
        res = enhance_cli.run(common + ["--outdir", str(tmp_path / mode)] + extra, model=m)
        assert res.n_done == 3
        outs[mode] = {name: (tmp_path / mode / f"{name}.wav").read_bytes() for name, _, _ in spec}
    assert outs["default"] == outs["host"] and outs["device"] == outs["device1"]
    assert outs["device"]["c"] == outs["host"]["c"] and outs["device"]["a"] != outs["host"]["a"]      # float32 rounding of the FIR
    jobs = list(enhance_cli.plan_jobs(sorted(str(p) for p in ind.glob("*.wav")), None, str(tmp_path / "o9"), None, None, True))
    for job, (name, n, sr) in zip(jobs, spec):
        y = resample_device(files[name].cuda(), sr, 48000)
        want = m.enhance(y, N=2, solver="euler", seed=[enhance_cli.clip_seed(11, job.index)])
        ref = tmp_path / f"ref_{name}.wav"
        enhance_cli.save_wav(str(ref), want.cpu(), 48000)
        assert outs["device"][name] == ref.read_bytes(), name
    # the host run writes what the host path gives: model.enhance on `resample`'s output
    y = enhance_cli.resample(files["b"], 44100, 48000)
    enhance_cli.save_wav(str(tmp_path / "ref_host.wav"), m.enhance(y, N=2, solver="euler", seed=[enhance_cli.clip_seed(11, jobs[1].index)]), 48000)
    assert outs["host"]["b"] == (tmp_path / "ref_host.wav").read_bytes()


def test_eval_cli_resample_device(tmp_path):
    from flowdec_amd import eval_cli
    from flowdec_amd.enhance_cli import save_wav
    from flowdec_amd.resample import resample_device
    rng = np.random.default_rng(22)
    n = 30000
    x = (0.1 * rng.standard_normal(n)).astype(np.float32)
    sigs = dict(clean=x, noisy=(x + 0.05 * rng.standard_normal(n)).astype(np.float32), enh=(x + 0.01 * rng.standard_normal(n)).astype(np.float32))
    for k, s in sigs.items():
        save_wav(str(tmp_path / f"{k}.wav"), torch.from_numpy(s), 44100)
    lst = tmp_path / "triples_list.txt"
    lst.write_text(" ---> ".join(str(tmp_path / f"{k}.wav") for k in ("clean", "noisy", "enh")) + "\n")
    res = eval_cli.run(["--triples", str(lst), "--out", str(tmp_path / "dev.csv"), "--resample", "device"])
    assert res.exit_code == 0 and res.n_scored == 1
    loaded = {k: eval_cli.load_mono(str(tmp_path / f"{k}.wav"), 48000, resample="device") for k in sigs}
    for k, s in sigs.items():
        assert loaded[k].is_cuda and torch.equal(loaded[k], resample_device(torch.from_numpy(s).cuda(), 44100, 48000, lowpass_filter_width=256))
    want = eval_cli.score([(loaded["enh"], loaded["clean"], loaded["noisy"])], 48000, 8, eval_cli.GPU_SCORER)
    row = (tmp_path / "dev.csv").read_text().strip().splitlines()[1].split(",")
    assert [float(v) for v in row[4:]] == [float(v) for v in want[0]] and np.isfinite(want).all()
    host = eval_cli.run(["--triples", str(lst), "--out", str(tmp_path / "host.csv")])
    # the same metrics up to the FIR's float32 rounding: the host output is within (K + 1) 2^-24 = 4e-5 of the signal's scale per sample; the
    # smallest energy formed, |e_art|^2, belongs to a component a tenth of that scale, so no ratio moves by more than 2 * 4e-4 -> 3.5e-3 dB
    np.testing.assert_allclose([m[1] for m in host.means[:3]], [m[1] for m in res.means[:3]], rtol=0, atol=1e-2)


def test_estimate_cli_resample_device(tmp_path):
    """Three 44.1 kHz pairs, shorter than the crop length at 48 kHz (padded: no random draw): the command line's estimate equals
    `estimate_params` on `resample_device`-loaded signals exactly."""
    import io
    from flowdec_amd import estimate as E, estimate_cli as CLI, eval_cli
    from flowdec_amd.enhance_cli import save_wav
    rng = np.random.default_rng(23)
    lines = []
    for i in range(3):
        x = (0.1 * rng.standard_normal(20000 + 100 * i)).astype(np.float32)
        y = (x + 0.02 * rng.standard_normal(len(x))).astype(np.float32)
        for k, s in (("clean", x), ("coded", y)):
            save_wav(str(tmp_path / f"{k}_{i}.wav"), torch.from_numpy(s), 44100)
        lines.append(f"{tmp_path / f'clean_{i}.wav'} ---> {tmp_path / f'coded_{i}.wav'}")
    pairs = tmp_path / "pairs.txt"
    pairs.write_text("\n".join(lines) + "\n")
    argv = ["--pairs-file", str(pairs), "--alpha", "0.3", "--nfft", "1534", "--hop", "384", "--n-samples", "3", "--sample-duration", "0.5", "--overwrite"]
    res = CLI.run(argv + ["--resample", "device"], out=io.StringIO())
    _, chosen = E.select_pairs(lines, 3, 302, " ---> ")
    xs, ys = [], []
    for fx, fy in chosen:
        x, y, start = E.crop_or_pad_pair(eval_cli.load_mono(fx, 48000, "device"), eval_cli.load_mono(fy, 48000, "device"), 24000)
        assert start is None and x.is_cuda and x.numel() == 24000
        xs.append(x); ys.append(y)
    want = E.estimate_params(xs, ys, alpha=0.3, n_fft=1534, hop=384)
    assert (res.beta, res.sigma_y, res.abs_quantile_x, res.rmse_quantile) == (want.beta, want.sigma_y, want.abs_quantile_x, want.rmse_quantile)
    assert np.isfinite([res.beta, res.sigma_y]).all() and res.beta > 0
