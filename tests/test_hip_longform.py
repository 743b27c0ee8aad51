"""Long-form enhance on the GPU (include/flowdec_hip.h "Long-form"; flowdec_amd/longform.py; FlowModel.enhance_long; --chunk-seconds).

Everything new reduces to something that exists, bit for bit: absolute-frame noise is a column slice of a wider fd_noise_fill plane;
fd_enhance_chunks with both arrays NULL is fd_enhance_seeded, with frame0 it is enhance(noise = that slice), with normfac_in it is the
per-row call on rows that share the file's peak; enhance_long of one row is enhance(seed=), of several rows the NumPy float32 stitch of
fd_enhance_chunks' rows.  Geometry throughout: the smallest model (nf = 8), rows of 64 frames, halos of 8, files of at most 4 rows, N = 2."""
import numpy as np
import pytest
import torch

import noise_oracle as NO
from conftest import rel_err
from oracle import flowdec_oracle as O

pytestmark = pytest.mark.gpu

HOP, NFFT, F = 384, 1534, 768
RF, HALO, X = 64, 8, 2 * HOP
W = RF * HOP - 1
STRIDE = (RF - 2 * HALO - 1) * HOP
N3 = 2 * STRIDE + W - 700          # three rows, the last shifted left by one hop (frame0 = 47 and 93: both odd)
N4 = 2 * STRIDE + W + 5            # four rows: the last starts ONE hop after the third
FRAME0S = (0, 1, 2, 63, 64, 2 ** 20 + 1)
_cache = {}


def _flow(precision, normalize_mode="noisy"):
    key = (precision, normalize_mode)
    if key not in _cache:
        import flowdec_amd
        m = flowdec_amd.from_preset("flowdec_75m", precision=precision, nf=8)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in O.random_state_dict(seed=8, nf=8).items()}, strict=False)
        m.normalize_mode = normalize_mode
        _cache[key] = m.cuda()
    return _cache[key]


def _file(n, seed=0, peak_rows=None):
    """A file of n samples in (-0.5, 0.5); peak_rows: the rows of its plan -- then 0.9 is planted in every row's kept range."""
    y = np.clip(0.1 * np.random.default_rng(seed).standard_normal(n), -0.5, 0.5).astype(np.float32)
    for j, r in enumerate(peak_rows or []):
        y[(r.keep[0] + r.keep[1]) // 2 + 7 * j] = 0.9 if j % 2 else -0.9
    return y


def _seed_tensor(vals):
    from flowdec_amd.noise import seeds_to_tensor
    return seeds_to_tensor(list(vals), len(vals), "cuda")


def _i32(vals):
    return torch.tensor(list(vals), dtype=torch.int32, device="cuda")


def _fill_at(seeds, frame0, F_, T, draw0=0, n_draws=1, bits=False):
    from flowdec_amd import _lib as L
    lib, s = L.load(), _seed_tensor(seeds)
    f0 = None if frame0 is None else _i32(frame0)
    B = len(seeds)
    if bits:
        raw = torch.empty(n_draws, B, F_, T, 2, dtype=torch.int32, device="cuda")
        L.check(lib.fd_noise_fill_at(L.ptr(raw), L.ptr(s), L.ptr(f0), B, F_, T, draw0, n_draws, 1, L.stream()))
        return (raw.to(torch.int64) & 0xFFFFFFFF).cpu().numpy()
    out = torch.empty(n_draws, B, F_, T, dtype=torch.complex64, device="cuda")
    L.check(lib.fd_noise_fill_at(L.ptr(torch.view_as_real(out)), L.ptr(s), L.ptr(f0), B, F_, T, draw0, n_draws, 0, L.stream()))
    return out


class Chunks:
    """fd_enhance_chunks / fd_enhance_seeded on buffers that keep their addresses (a captured graph is keyed on them)."""

    def __init__(self, m, B, Lrow):
        from flowdec_amd import _lib as L
        self.L, self.lib, self.m, self.B, self.Lrow = L, L.load(), m, B, Lrow
        self.h = m._sync_native()
        self.y = torch.zeros(B, Lrow, device="cuda")
        self.out = torch.empty(B, Lrow, device="cuda")
        self.lens, self.frame0 = _i32([Lrow] * B), _i32([0] * B)
        self.seeds = torch.zeros(B, dtype=torch.int64, device="cuda")
        self.normfac = torch.ones(B, device="cuda")
        self.ws = torch.empty(self.lib.fd_enhance_workspace_bytes(self.h, B, Lrow), dtype=torch.uint8, device="cuda")
        self.stream = torch.cuda.Stream()

    def load(self, clips, seeds, frame0=None, normfac=None):
        self.y.zero_()
        for b, c in enumerate(clips):
            self.y[b, :len(c)] = torch.as_tensor(c)
        self.lens.copy_(_i32([len(c) for c in clips]))
        self.seeds.copy_(_seed_tensor(seeds))
        if frame0 is not None:
            self.frame0.copy_(_i32(frame0))
        if normfac is not None:
            self.normfac.copy_(torch.as_tensor(normfac, dtype=torch.float32))
        return self

    def run(self, frame0=False, normfac=False, seeded=False, use_graph=False, N=2, solver="euler"):
        L, lib = self.L, self.lib
        self.h = self.m._sync_native()
        torch.cuda.synchronize()
        with torch.cuda.stream(self.stream):
            tail = (1.0, N, L.SOLVERS[solver], L.ptr(self.out), self.B, self.Lrow, L.ptr(self.ws), self.ws.numel(), int(use_graph), L.stream())
            if seeded:
                L.check(lib.fd_enhance_seeded(self.h, L.ptr(self.y), L.ptr(self.lens), L.ptr(self.seeds), *tail))
            else:
                L.check(lib.fd_enhance_chunks(self.h, L.ptr(self.y), L.ptr(self.lens), L.ptr(self.seeds), L.ptr(self.frame0) if frame0 else None,
                                              L.ptr(self.normfac) if normfac else None, *tail))
        self.stream.synchronize()
        return self.out.clone()

    def front_end(self):
        """Y [B, 1, F, T_pad]: the compressed spectrogram the front end left at the start of the workspace."""
        Tp = self.lib.fd_padded_frames(self.lib.fd_num_frames(self.Lrow, HOP))
        return torch.view_as_complex(self.ws[:self.B * F * Tp * 8].view(torch.float32).reshape(self.B, 1, F, Tp, 2)).cpu().numpy()


def _normfac(y_rows, lengths=None):
    from flowdec_amd import _lib as L
    y = torch.as_tensor(y_rows, device="cuda").reshape(-1, np.shape(y_rows)[-1]).contiguous()
    out = torch.empty(y.shape[0], device="cuda")
    lens = None if lengths is None else _i32(lengths)
    L.check(L.load().fd_normfac(L.ptr(y), L.ptr(lens), y.shape[0], y.shape[1], L.ptr(out), L.stream()))
    return out


def _plan(n, xfade=X):
    from flowdec_amd.longform import plan_rows
    return plan_rows(n, HOP, RF, HALO, xfade)


def _row_outputs(m, y, rows, seed, normalize):
    """Every row's output through fd_enhance_chunks, ONE row per call."""
    ch = Chunks(m, 1, W)
    nf = _normfac(y[None]).cpu().numpy() if normalize else None
    outs = []
    for r in rows:
        ch.load([y[r.start:r.start + r.length]], [seed], [r.frame0], nf)
        outs.append(ch.run(frame0=True, normfac=normalize)[0, :r.length].cpu().numpy())
    return outs


# ---- 1. absolute-frame noise, bits exact ---------------------------------------------------------------------------------
def test_noise_fill_at_bits_equal_oracle_at_absolute_frames():
    """Every offset on its own and paired with another one in one call (two rows, different offsets); F = 3, T_pad = 64; draws 2 and 3."""
    seeds = (1000, (1 << 63) + 1001)
    for f0 in [(a, b) for a, b in zip(FRAME0S, FRAME0S[1:] + FRAME0S[:1])]:
        got = _fill_at(seeds, f0, 3, 64, draw0=2, n_draws=2, bits=True)
        assert got.shape == (2, 2, 3, 64, 2)
        for d in range(2):
            for b, s in enumerate(seeds):
                ra, rb = NO.noise_bits(s, 2 + d, 3, f0[b] + 64)
                assert np.array_equal(got[d, b, :, :, 0], ra[:, f0[b]:].astype(np.int64)), (f0, d, b, "ra")
                assert np.array_equal(got[d, b, :, :, 1], rb[:, f0[b]:].astype(np.int64)), (f0, d, b, "rb")


def test_noise_fill_at_is_a_column_slice_of_a_wider_plane():
    """Gaussian and bits mode == columns [frame0, frame0 + T_pad) of fd_noise_fill with a larger T_pad, for every offset incl. 2^20 + 1; an odd
    T_pad; NULL == fd_noise_fill."""
    from flowdec_amd.noise import noise_fill
    seeds = (7, 8)
    small = [f for f in FRAME0S if f < 2 ** 20]
    wide = noise_fill(_seed_tensor(seeds), 3, 64 + 64 + 1, 0, 2)[:, :, 0]                 # [2, B, 3, 129]
    wide_bits = noise_fill(_seed_tensor(seeds), 3, 64 + 64 + 1, 0, 2, bits=True)[:, :, 0].cpu().numpy()
    for a, b in zip(small, small[1:] + small[:1]):
        for T in (64, 63):
            z = _fill_at(seeds, (a, b), 3, T, 0, 2)
            zb = _fill_at(seeds, (a, b), 3, T, 0, 2, bits=True)
            for i, f0 in enumerate((a, b)):
                assert torch.equal(torch.view_as_real(z[:, i]), torch.view_as_real(wide[:, i, :, f0:f0 + T])), (a, b, T, i)
                assert np.array_equal(zb[:, i], wide_bits[:, i, :, f0:f0 + T]), (a, b, T, i)
    # the far offset, next to a near one in the same call: a plane of 2^20 + 65 columns (F = 3: 25 MB per row), sliced on the device
    far = 2 ** 20 + 1
    wide = noise_fill(_seed_tensor(seeds), 3, far + 64)[0, :, 0]                          # [B, 3, 2^20 + 65]
    wide_bits = noise_fill(_seed_tensor(seeds), 3, far + 64, bits=True)[0, :, 0]
    z, zb = _fill_at(seeds, (far, 63), 3, 64)[0], _fill_at(seeds, (far, 63), 3, 64, bits=True)[0]
    for i, f0 in enumerate((far, 63)):
        assert torch.equal(torch.view_as_real(z[i]), torch.view_as_real(wide[i, :, f0:f0 + 64])), f0
        assert np.array_equal(zb[i], wide_bits[i, :, f0:f0 + 64].cpu().numpy()), f0
    del wide, wide_bits
    # ... and its Gaussians from the oracle's bits of those frames (float64, the tolerance of tests/test_hip_noise.py: 1e-5)
    z = _fill_at(seeds[:1], (far,), 3, 64)[0, 0].cpu().numpy()
    ra, rb = NO.noise_bits(seeds[0], 0, 3, far + 64)
    ref = NO.gaussian_from_bits(ra[:, far:], rb[:, far:])
    assert np.abs(z - ref).max() < 1e-5
    for bits in (False, True):
        a = _fill_at(seeds, None, F, 64, 1, 2, bits=bits)
        b = noise_fill(_seed_tensor(seeds), F, 64, 1, 2, bits=bits)[:, :, 0]
        assert np.array_equal(a, b.cpu().numpy()) if bits else torch.equal(torch.view_as_real(a), torch.view_as_real(b))
        assert (a if bits else a.cpu().numpy()).any()


# ---- 2. the file's normalisation factor -------------------------------------------------------------------------------------
def test_normfac_rule():
    rng = np.random.default_rng(1)
    y = rng.standard_normal((5, 70001)).astype(np.float32)
    y[1] = 0.0                               # silence: isclose(0) -> 1
    y[2] *= 1e-9                             # max <= 1e-8 -> 1
    y[3, -1] = -7.5                          # the peak in the last sample, negative
    lens = [70001, 70001, 70001, 70001, 1]   # a row of ONE sample
    want = [np.abs(y[0]).max(), 1.0, 1.0, 7.5, abs(y[4, 0])]
    assert np.array_equal(_normfac(y, lens).cpu().numpy(), np.array(want, dtype=np.float32))
    assert np.array_equal(_normfac(y).cpu().numpy()[[0, 3]], np.array([want[0], 7.5], dtype=np.float32))
    lens[3] = 70000                          # ... and not counted when the length stops before it
    assert _normfac(y, lens)[3].item() == np.abs(y[3, :70000]).max()


# ---- 3. fd_enhance_chunks reduces to what exists -------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_chunks_with_null_arrays_is_enhance_seeded(precision):
    m = _flow(precision)
    y = _file(N3, seed=2)
    clips = [y[:W], y[5000:5000 + W - 700], y[9000:9000 + W - 383]]                  # ragged rows of the 64-frame bucket
    ch = Chunks(m, 3, W).load(clips, [11, (1 << 63) + 12, 13])
    ref = ch.run(seeded=True)
    assert torch.isfinite(ref).all() and ref.abs().max() > 0
    assert torch.equal(ch.run(), ref), "eager: fd_enhance_chunks(NULL, NULL) != fd_enhance_seeded"
    assert torch.equal(ch.run(solver="midpoint"), ch.run(seeded=True, solver="midpoint"))
    for i in range(3):                                                               # eager, captured, replayed
        assert torch.equal(ch.run(use_graph=True), ref), f"graph call {i}"


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_chunks_frame0_rows_equal_enhance_on_the_noise_slice(precision):
    """normalize_mode='none'.  Row k of a 3-row file == enhance(row k's samples, noise = columns [frame0_k, frame0_k + 64) of the whole
    file's fd_noise_fill plane); the three rows in one call and one by one; eager and graph."""
    from flowdec_amd.noise import noise_fill
    m = _flow(precision, "none")
    rows = _plan(N3)
    assert len(rows) == 3 and rows[2].frame0 % 2 == 1 and rows[1].frame0 % 2 == 1, [r.frame0 for r in rows]    # odd offsets
    y = _file(N3, seed=3)
    seed = 0xDEADBEEFCAFEF00D
    plane = noise_fill(_seed_tensor([seed]), F, rows[-1].frame0 + RF)[0]             # [1, 1, F, T of the file]
    refs = []
    for r in rows:
        nz = plane[..., r.frame0:r.frame0 + RF].contiguous()
        refs.append(m.enhance(torch.from_numpy(y[r.start:r.start + r.length]), N=2, solver="euler", noise=nz, use_graph=False))
    assert all(torch.isfinite(x).all() and x.abs().max() > 0 for x in refs)
    ch = Chunks(m, 3, W).load([y[r.start:r.start + r.length] for r in rows], [seed] * 3, [r.frame0 for r in rows])
    out = ch.run(frame0=True)
    for k, r in enumerate(rows):
        assert torch.equal(out[k, :r.length].cpu(), refs[k]), f"row {k} (frame0 {r.frame0})"
        assert not out[k, r.length:].any()
    assert not torch.equal(ch.run(), out), "frame0 has no effect"
    for i in range(3):
        assert torch.equal(ch.run(frame0=True, use_graph=True), out), f"graph call {i}"
    for k, o in enumerate(_row_outputs(m, y, rows, seed, normalize=False)):
        assert np.array_equal(o, refs[k].numpy()), f"row {k} alone"


def test_chunks_normfac_in():
    """'noisy' model, the same peak planted in every row: each row == the existing per-row call (whose own maximum is that peak).  Then
    the front end alone with arbitrary factors against the NumPy oracle's STFT + compression."""
    from flowdec_amd.noise import noise_fill
    m = _flow("fp32")
    rows = _plan(N3)
    y = _file(N3, seed=4, peak_rows=rows)
    nf = _normfac(y[None])
    assert nf.item() == np.float32(0.9)
    seed = 77
    plane = noise_fill(_seed_tensor([seed]), F, rows[-1].frame0 + RF)[0]
    clips = [y[r.start:r.start + r.length] for r in rows]
    ch = Chunks(m, 3, W).load(clips, [seed] * 3, [r.frame0 for r in rows], nf.expand(3))
    out = ch.run(frame0=True, normfac=True)
    for k, r in enumerate(rows):
        assert np.abs(clips[k]).max() == np.float32(0.9)
        ref = m.enhance(torch.from_numpy(clips[k]), N=2, solver="euler", noise=plane[..., r.frame0:r.frame0 + RF].contiguous(), use_graph=False)
        assert torch.equal(out[k, :r.length].cpu(), ref), f"row {k}"
    for i in range(3):
        assert torch.equal(ch.run(frame0=True, normfac=True, use_graph=True), out), f"graph call {i}"
    # arbitrary factors: Y = compress(stft(y / factor)), zero-padded to 64 frames, at the project's 2e-5; the output scales back by it
    factors = [1.7, 0.3, 0.9]
    ch.load(clips, [seed] * 3, [r.frame0 for r in rows], factors)
    scaled = ch.run(frame0=True, normfac=True)
    Y = ch.front_end()
    for k, c in enumerate(clips):
        ref = O.pad_spec(O.compress(O.stft((c.astype(np.float64) / np.float64(np.float32(factors[k])))[None, None])))[0]
        e = rel_err(Y[k:k + 1], ref)
        print(f"front end with normfac_in = {factors[k]}: rel err {e:.3e}")
        assert e < 2e-5, (k, e)
    assert torch.isfinite(scaled).all() and not torch.equal(scaled[0], out[0]) and torch.equal(scaled[2], out[2])


# ---- 4. stitching ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,xfade", [(N3, X), (N4, X), (N4, 0), (N4, 2), (W + 1, 2 * HALO * HOP)])
def test_stitch_kernel_equals_numpy_float32(n, xfade):
    from flowdec_amd import _lib as L
    from flowdec_amd.longform import stitch_reference, stitch_weights
    rows = _plan(n, xfade)
    rng = np.random.default_rng(n % 1000 + xfade)
    outs = [rng.standard_normal(r.length).astype(np.float32) for r in rows]          # unrelated rows: every weight matters
    buf = torch.full((len(rows), W), float("nan"), device="cuda")
    for j, o in enumerate(outs):
        buf[j, :len(o)] = torch.from_numpy(o)
    got = torch.empty(n, device="cuda")
    w = torch.from_numpy(stitch_weights(xfade)).cuda() if xfade else None
    starts, bounds = _i32([r.start for r in rows]), _i32([r.xfade_lo for r in rows[1:]])
    L.check(L.load().fd_stitch_chunks(L.ptr(buf), W, L.ptr(starts), L.ptr(bounds), len(rows), L.ptr(w), xfade, L.ptr(got), n, L.stream()))
    assert np.array_equal(got.cpu().numpy(), stitch_reference(outs, rows, xfade))


# ---- 5. enhance_long --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_enhance_long_one_row_is_enhance_seeded(precision):
    m = _flow(precision)
    for n, kw in ((20000, dict(row_frames=RF, halo_frames=HALO)), (W, dict(row_frames=RF, halo_frames=HALO)), (30000, {})):
        y = torch.from_numpy(_file(n, seed=n))
        ref = m.enhance(y, N=2, solver="midpoint", seed=5)
        assert torch.isfinite(ref).all() and ref.abs().max() > 0
        out = m.enhance_long(y, N=2, solver="midpoint", seed=5, **kw)
        assert out.shape == y.shape and out.device == y.device and torch.equal(out, ref), (n, kw)
    assert torch.equal(m.enhance_long(y[None, None].cuda(), N=2, solver="midpoint", seed=5), ref[None, None].cuda())


@pytest.mark.parametrize("precision,n", [("bf16", N4), ("fp32", N3)])
def test_enhance_long_is_the_float32_stitch_of_its_rows(precision, n):
    from flowdec_amd.longform import stitch_reference
    from flowdec_amd.noise import clip_seed
    m = _flow(precision)
    rows = _plan(n)
    assert len(rows) == (4 if n == N4 else 3)
    y = _file(n, seed=6)
    want = stitch_reference(_row_outputs(m, y, rows, clip_seed(9, 0), normalize=True), rows, X)
    assert np.isfinite(want).all() and np.abs(want).max() > 0
    for rpc in (1, 2, 8):
        got = m.enhance_long(torch.from_numpy(y), N=2, seed=9, row_frames=RF, halo_frames=HALO, rows_per_call=rpc)
        assert np.array_equal(got.numpy(), want), f"rows_per_call = {rpc}"
    eager = m.enhance_long(torch.from_numpy(y), N=2, seed=9, row_frames=RF, halo_frames=HALO, rows_per_call=2, use_graph=False)
    assert np.array_equal(eager.numpy(), want)
    other = m.enhance_long(torch.from_numpy(y), N=2, seed=10, row_frames=RF, halo_frames=HALO)
    assert not np.array_equal(other.numpy(), want)
    # normalize_mode='none' passes no factor
    mn = _flow(precision, "none")
    want = stitch_reference(_row_outputs(mn, y, rows, clip_seed(9, 0), normalize=False), rows, X)
    assert np.array_equal(mn.enhance_long(torch.from_numpy(y), N=2, seed=9, row_frames=RF, halo_frames=HALO).numpy(), want)


def test_enhance_long_two_channels_are_two_files():
    m = _flow("bf16")
    y = torch.from_numpy(np.stack([_file(N3, seed=11), 3 * _file(N3, seed=12)]))[:, None]            # [2, 1, n], different levels
    kw = dict(N=2, row_frames=RF, halo_frames=HALO)
    both = m.enhance_long(y, seed=[21, 22], **kw)
    assert both.shape == y.shape
    for c, s in enumerate((21, 22)):
        assert torch.equal(both[c, 0], m.enhance_long(y[c, 0], seed=[s], **kw)), f"channel {c}"
    from flowdec_amd.noise import clip_seed
    assert torch.equal(m.enhance_long(y, seed=4, **kw), m.enhance_long(y, seed=[clip_seed(4, 0), clip_seed(4, 1)], **kw))
    a, b = m.enhance_long(y[0, 0], **kw), m.enhance_long(y[0, 0], **kw)                                # seed=None: drawn from torch's generator
    assert torch.isfinite(a).all() and not torch.equal(a, b)
    with pytest.raises(ValueError):
        m.enhance_long(y, solver="tsit5", **kw)
    with pytest.raises(RuntimeError):
        m.enhance_long(y, seed=[1], **kw)                                                              # one seed per channel


def test_forty_rows_in_the_workspace_of_eight():
    """A 40-row file runs in 5 calls of 8 rows: afterwards the model holds the (8, W) workspace and nothing larger, and the one-shot call
    on the same length would need several times that (both figures from fd_enhance_workspace_bytes: computed, not measured)."""
    from flowdec_amd import _lib as L
    m = _flow("bf16")
    n = 39 * STRIDE + W - 100
    assert len(_plan(n)) == 40
    m.backbone.invalidate()                                                                            # drop the workspaces of earlier tests
    y = torch.from_numpy(_file(n, seed=13))
    out = m.enhance_long(y, N=2, seed=1, row_frames=RF, halo_frames=HALO, rows_per_call=8)
    assert out.shape == y.shape and torch.isfinite(out).all() and out.abs().max() > 0
    lib, h = L.load(), m._sync_native()
    rows8, one_shot = lib.fd_enhance_workspace_bytes(h, 8, W), lib.fd_enhance_workspace_bytes(h, 1, n)
    print(f"40 rows: workspace of (8, {W}) = {rows8 / 2**20:.1f} MiB; one shot of {n} samples = {one_shot / 2**20:.1f} MiB")
    assert set(m.backbone._ws) == {"enh"} and m.backbone._ws["enh"].numel() == rows8
    assert one_shot > 3 * rows8
    assert torch.equal(out, m.enhance_long(y, N=2, seed=1, row_frames=RF, halo_frames=HALO, rows_per_call=5))
    assert m.backbone._ws["enh"].numel() == rows8, "a smaller group reuses the buffer"


# ---- 6. the command line -----------------------------------------------------------------------------------------------------------
def test_cli_chunk_seconds(tmp_path):
    from test_cli import synthetic_ckpt
    from flowdec_amd import enhance_cli, longform
    from flowdec_amd.noise import clip_seed
    torch.save(synthetic_ckpt(), tmp_path / "m.ckpt")
    ind = tmp_path / "in"
    ind.mkdir()
    spec = [("a", 24000), ("b", 20000), ("long", 60000), ("z", 23000)]
    for i, (name, n) in enumerate(spec):
        enhance_cli.save_wav(str(ind / f"{name}.wav"), torch.from_numpy(_file(n, seed=20 + i))[None], 48000)
    # --max-seconds 1: `long` (1.25 s) is over the length rule; --chunk-seconds 0.6 -> rows of 64 frames (0.51 s), halos of 16
    common = ["--ckpt", str(tmp_path / "m.ckpt"), "--files", str(ind), "--N", "2", "--solver", "midpoint", "--rng", "native", "--seed", "3",
              "--max-seconds", "1", "--rtf"]
    off = enhance_cli.run(common + ["--outdir", str(tmp_path / "off")])
    on = enhance_cli.run(common + ["--outdir", str(tmp_path / "on"), "--chunk-seconds", "0.6"])
    assert (off.n_done, off.n_too_long) == (3, 1) and not (tmp_path / "off" / "long.wav").exists()
    assert (on.n_done, on.n_too_long) == (4, 0)
    for name in ("a", "b", "z"):
        assert (tmp_path / "on" / f"{name}.wav").read_bytes() == (tmp_path / "off" / f"{name}.wav").read_bytes(), name
    assert longform.chunk_row_frames(0.6, 48000, HOP) == 64 and len(longform.plan_rows(60000, HOP, 64, 16)) == 4
    m = enhance_cli.load_from_checkpoint(str(tmp_path / "m.ckpt"), map_location="cuda:0")
    y, _ = enhance_cli.load_wav(str(ind / "long.wav"))
    want = m.enhance_long(y, N=2, solver="midpoint", seed=[clip_seed(3, 2)], row_frames=64, halo_frames=16)     # `long` is file 2 of the work list
    enhance_cli.save_wav(str(tmp_path / "want.wav"), want, 48000)
    assert (tmp_path / "on" / "long.wav").read_bytes() == (tmp_path / "want.wav").read_bytes()
    rtf = (tmp_path / "on" / "rtfs.csv").read_text().strip().splitlines()[1:]
    assert sorted(l.split(",")[0].split("/")[-1] for l in rtf) == ["a.wav", "b.wav", "long.wav", "z.wav"]          # its own row
