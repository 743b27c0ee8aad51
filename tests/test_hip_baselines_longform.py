"""Long-form for the ScoreDec and regression baselines on the GPU (include/flowdec_hip.h "Long-form", "Seeded noise"; fd_caxpy_at,
fd_score_update_at, fd_score_enhance_chunks, fd_regression_enhance_chunks; _WaveModel._enhance_long).

As in tests/test_hip_longform.py everything new reduces to something that exists, bit for bit: the operators at absolute frames are the
unseeded operators on the fd_noise_fill_at plane; the chunks calls with NULL arrays are the ragged calls, with frame0 they are
enhance(noise = the planes at those frames), with normfac_in the per-row call on rows that share the file's peak; the long form of one row
is enhance(seed=), of several rows the NumPy float32 stitch of the rows run one per call.  Geometry of that file: nf = 8, rows of 64
frames, halos of 8, files of at most 4 rows, N = 2.

The public name `enhance_long` of the two baseline classes is pinned absent by tests/test_longform_cpu.py; the tests call the base
class's machinery (`_enhance_long` with the class's `_chunks_call`), which FlowModel.enhance_long and the streaming pools run too."""
import ctypes as C

import numpy as np
import pytest
import torch

import solver_ops_ref as R
from test_hip_baselines import baseline
from test_hip_longform import F, FRAME0S, HALO, HOP, N3, N4, RF, W, X, _file, _fill_at, _i32, _normfac, _plan, _seed_tensor

pytestmark = pytest.mark.gpu

PC = dict(predictor="reverse_diffusion", corrector="ald", N=2, corrector_steps=1, snr=0.5, denoise=True)        # 5 draws
EM = dict(predictor="euler_maruyama", corrector="none", N=2, corrector_steps=1, snr=0.5, denoise=False)        # 3 draws
GEO = dict(row_frames=RF, halo_frames=HALO)
TRIPLES = (FRAME0S[:3], FRAME0S[3:])          # (0, 1, 2) and (63, 64, 2^20 + 1): B = 3 rows each


def plane(a):
    return torch.view_as_complex(torch.from_numpy(np.ascontiguousarray(a, np.float32))).cuda()


def back(t):
    return torch.view_as_real(t).cpu().numpy()


def nans(*shape):
    return plane(R.sentinel(tuple(shape) + (2,)))


def long_form(m, y, seed=None, normfac=None, rows_per_call=8, use_graph=True, **sampler):
    """What `enhance_long(y, <sampler>, seed=, row_frames=64, halo_frames=8, ...)` is for the class of `m`."""
    return m._enhance_long(y, m._chunks_call(**sampler), seed=seed, rows_per_call=rows_per_call, use_graph=use_graph, normfac=normfac, **GEO)


# ---- 1. the operators at absolute frames ------------------------------------------------------------------------------------------------
def test_caxpy_at():
    """NULL frame0 == fd_op_caxpy; with frame0 == the unseeded operator on the fd_noise_fill_at plane of that draw (draws 0 and 3), bit for
    bit: odd offsets (a thread's frame on the second word pair of a Philox call) and 2^20 + 1 (no index folded into the row width)."""
    from flowdec_amd import ops
    B, Fq, T = 3, 3, 64
    seeds = (5, (1 << 63) + 6, 7)
    st = _seed_tensor(seeds)
    a = plane(R.plane_data(np.random.default_rng(0), (B, Fq, T), False)[0])
    for draw in (0, 3):
        plain = back(ops.caxpy(a, -1.37, seeds=st, draw=draw, out=nans(B, Fq, T)))
        assert np.isfinite(plain).all()
        assert R.same_bits(back(ops.caxpy(a, -1.37, seeds=st, draw=draw, out=nans(B, Fq, T), at=True)), plain), f"draw {draw}: NULL frame0"
        assert R.same_bits(back(ops.caxpy(a, -1.37, seeds=st, draw=draw, out=nans(B, Fq, T), frame0=_i32([0, 0, 0]))), plain), f"draw {draw}: zeros"
        q = plane(R.plane_data(np.random.default_rng(1), (B, Fq, T), False)[1])
        assert R.same_bits(back(ops.caxpy(a, 0.5, q=q, out=nans(B, Fq, T), at=True)), back(ops.caxpy(a, 0.5, q=q, out=nans(B, Fq, T))))
        for f0 in TRIPLES:
            z = _fill_at(seeds, f0, Fq, T, draw0=draw)[0].contiguous()
            got = back(ops.caxpy(a, -1.37, seeds=st, draw=draw, out=nans(B, Fq, T), frame0=_i32(f0)))
            assert R.same_bits(got, back(ops.caxpy(a, -1.37, q=z, out=nans(B, Fq, T)))), (draw, f0)
            if f0[0]:
                assert not R.same_bits(got, plain), (draw, f0, "frame0 has no effect")


@pytest.mark.parametrize("ks", [1, 3])
@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_score_update_at(dtype, ks):
    """The same three statements for the fused predictor / corrector update; and with cz == 0 the result does not depend on what frame0
    holds (the noise term is skipped: neither seeds nor frame0 is consulted)."""
    from flowdec_amd import ops
    rng = np.random.default_rng(10 + ks)
    shape = B, H, Wd = 3, 3, 64
    seeds = (0x1234567890ABCDEF, 42, (1 << 63) + 9)
    st = _seed_tensor(seeds)
    w = R.output_weights(rng, ks, False)
    pyr, (base, Y, _, _) = R.image_data(rng, shape, dtype, False)
    dpyr = torch.from_numpy(np.ascontiguousarray(pyr, np.float32)).cuda().to({"bf16": torch.bfloat16, "fp32": torch.float32}[dtype])
    dw, dbase, dY = torch.from_numpy(w).cuda(), plane(base), plane(Y)
    co = (0.93, dY, 0.071, -0.013)

    def upd(cz=0.37, **kw):
        return back(ops.score_update(dpyr, dw, dbase, co[0], co[1], co[2], co[3], cz, dst=nans(*shape), **kw))

    for draw in (0, 3):
        plain = upd(seeds=st, draw=draw)
        assert np.isfinite(plain).all()
        assert R.same_bits(upd(seeds=st, draw=draw, at=True), plain), f"draw {draw}: NULL frame0"
        for f0 in TRIPLES:
            z = _fill_at(seeds, f0, H, Wd, draw0=draw)[0].contiguous()
            got = upd(seeds=st, draw=draw, frame0=_i32(f0))
            assert R.same_bits(got, upd(z=z)), (draw, f0)
            if f0[0]:
                assert not R.same_bits(got, plain), (draw, f0, "frame0 has no effect")
    quiet = upd(cz=0.0)
    garbage = _i32([2 ** 31 - 1, -(2 ** 31), 12345])
    assert R.same_bits(upd(cz=0.0, seeds=st, draw=3, frame0=garbage), quiet) and np.isfinite(quiet).all()


# ---- 2. fd_score_enhance_chunks / fd_regression_enhance_chunks -----------------------------------------------------------------------------
class Chunks:
    """The baselines' chunks / ragged calls on buffers that keep their addresses (a captured graph is keyed on them)."""

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

    def load(self, clips, seeds=None, frame0=None, normfac=None):
        self.y.zero_()
        for b, c in enumerate(clips):
            self.y[b, :len(c)] = torch.as_tensor(c)
        self.lens.copy_(_i32([len(c) for c in clips]))
        if seeds is not None:
            self.seeds.copy_(_seed_tensor(seeds))
        if frame0 is not None:
            self.frame0.copy_(_i32(frame0))
        if normfac is not None:
            self.normfac.copy_(torch.as_tensor(normfac, dtype=torch.float32))
        return self

    def run(self, sampler=None, frame0=False, normfac=False, ragged=False, use_graph=False):
        """sampler: the score model's (None: the regression calls); ragged: the existing *_ragged entry point."""
        L, lib = self.L, self.lib
        self.h = self.m._sync_native()
        torch.cuda.synchronize()
        with torch.cuda.stream(self.stream):
            tail = (L.ptr(self.out), self.B, self.Lrow, L.ptr(self.ws), self.ws.numel(), int(use_graph), L.stream())
            f0, nf = L.ptr(self.frame0) if frame0 else None, L.ptr(self.normfac) if normfac else None
            if sampler is None:
                if ragged:
                    L.check(lib.fd_regression_enhance_ragged(self.h, L.ptr(self.y), L.ptr(self.lens), *tail))
                else:
                    L.check(lib.fd_regression_enhance_chunks(self.h, L.ptr(self.y), L.ptr(self.lens), nf, *tail))
            else:
                cfg, _ = self.m._pc_config(**sampler)
                if ragged:
                    L.check(lib.fd_score_enhance_ragged(self.h, L.ptr(self.y), L.ptr(self.lens), None, L.ptr(self.seeds), C.byref(cfg), *tail))
                else:
                    L.check(lib.fd_score_enhance_chunks(self.h, L.ptr(self.y), L.ptr(self.lens), L.ptr(self.seeds), f0, nf, C.byref(cfg), *tail))
        self.stream.synchronize()
        return self.out.clone()


def _ragged_clips(seed):
    y = _file(N3, seed=seed)
    return [y[:W], y[5000:5000 + W - 700], y[9000:9000 + W - 383]]                   # ragged rows of the 64-frame bucket


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_score_chunks_with_null_arrays_is_score_enhance_ragged(precision):
    m = baseline("score", precision)
    ch = Chunks(m, 3, W).load(_ragged_clips(2), [11, (1 << 63) + 12, 13])
    ref = ch.run(PC, ragged=True)
    assert torch.isfinite(ref).all() and ref.abs().max() > 0
    assert torch.equal(ch.run(PC), ref), "eager: fd_score_enhance_chunks(NULL, NULL) != fd_score_enhance_ragged(seeds)"
    assert torch.equal(ch.run(EM), ch.run(EM, ragged=True)) and not torch.equal(ch.run(EM), ref)
    for i in range(3):                                                               # eager, captured, replayed
        assert torch.equal(ch.run(PC, use_graph=True), ref), f"graph call {i}"
    # the graph is keyed on the POINTERS: new contents of seeds and frame0, in place, reach the next replay
    at = ch.run(PC, frame0=True, use_graph=True)
    assert torch.equal(at, ref), "frame0 = zeros"
    ch.load(_ragged_clips(2), [21, 22, 23], [47, 93, 1])
    moved = ch.run(PC, frame0=True, use_graph=True)
    assert torch.equal(moved, ch.run(PC, frame0=True)) and not torch.equal(moved, ref), "a replay after seeds / frame0 changed in place"


@pytest.mark.parametrize("sampler", [PC, EM], ids=["rd_ald_denoise", "em_none"])
@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_score_chunks_frame0_rows_equal_enhance_on_the_noise_planes(precision, sampler):
    """normalize_mode='none'.  Row k of the 3-row file N3 (row starts at frames 47 and 93: odd) == ScoreModel.enhance(row, noise = the
    fd_noise_fill_at planes of ALL fd_score_num_draws draws at that row's frame0); three rows in one call, eager and graph."""
    m = baseline("score", precision)
    mode, m.normalize_mode = m.normalize_mode, "none"
    try:
        rows = _plan(N3)
        assert [r.frame0 for r in rows[1:]] == [47, 93]
        y = _file(N3, seed=3)
        seed = 0xDEADBEEFCAFEF00D
        n = m.num_draws(sampler["N"], sampler["predictor"], sampler["corrector"], sampler["corrector_steps"])
        assert n == (5 if sampler is PC else 3)
        refs = []
        for r in rows:
            planes = _fill_at([seed], [r.frame0], F, RF, 0, n)[:, :, None].contiguous()            # [n, 1, 1, F, 64]
            refs.append(m.enhance(torch.from_numpy(y[r.start:r.start + r.length]), noise=planes, use_graph=False, **sampler))
        assert all(torch.isfinite(x).all() and x.abs().max() > 0 for x in refs)
        ch = Chunks(m, 3, W).load([y[r.start:r.start + r.length] for r in rows], [seed] * 3, [r.frame0 for r in rows])
        out = ch.run(sampler, frame0=True)
        for k, r in enumerate(rows):
            assert torch.equal(out[k, :r.length].cpu(), refs[k]), f"row {k} (frame0 {r.frame0})"
            assert not out[k, r.length:].any()
        assert not torch.equal(ch.run(sampler), out), "frame0 has no effect"
        for i in range(2):
            assert torch.equal(ch.run(sampler, frame0=True, use_graph=True), out), f"graph call {i}"
    finally:
        m.normalize_mode = mode


def test_chunks_normfac_in_both_classes():
    """'noisy' models, the same peak planted in every row's kept range: each row == the existing per-row call (whose own maximum is that
    peak); another factor scales the row, the file's own does not."""
    rows = _plan(N3)
    y = _file(N3, seed=4, peak_rows=rows)
    nf = _normfac(y[None])
    assert nf.item() == np.float32(0.9)
    clips = [y[r.start:r.start + r.length] for r in rows]
    assert all(np.abs(c).max() == np.float32(0.9) for c in clips)
    seed = 77
    ms, mr = baseline("score", "fp32"), baseline("regression", "fp32")
    n = ms.num_draws(2)
    ch = Chunks(ms, 3, W).load(clips, [seed] * 3, [r.frame0 for r in rows], nf.expand(3))
    out = ch.run(PC, frame0=True, normfac=True)
    for k, r in enumerate(rows):
        planes = _fill_at([seed], [r.frame0], F, RF, 0, n)[:, :, None].contiguous()
        assert torch.equal(out[k, :r.length].cpu(), ms.enhance(torch.from_numpy(clips[k]), noise=planes, use_graph=False, **PC)), f"score row {k}"
    for i in range(2):
        assert torch.equal(ch.run(PC, frame0=True, normfac=True, use_graph=True), out), f"score graph call {i}"
    scaled = ch.load(clips, normfac=[1.7, 0.3, 0.9]).run(PC, frame0=True, normfac=True)
    assert torch.isfinite(scaled).all() and not torch.equal(scaled[0], out[0]) and torch.equal(scaled[2], out[2])
    cr = Chunks(mr, 3, W).load(clips, normfac=nf.expand(3))
    out = cr.run(normfac=True)
    for k, r in enumerate(rows):
        assert torch.equal(out[k, :r.length].cpu(), mr.enhance(torch.from_numpy(clips[k]), use_graph=False)), f"regression row {k}"
    for i in range(2):
        assert torch.equal(cr.run(normfac=True, use_graph=True), out), f"regression graph call {i}"
    scaled = cr.load(clips, normfac=[1.7, 0.3, 0.9]).run(normfac=True)
    assert torch.isfinite(scaled).all() and not torch.equal(scaled[0], out[0]) and torch.equal(scaled[2], out[2])


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_regression_chunks_with_null_normfac_is_regression_enhance_ragged(precision):
    m = baseline("regression", precision)
    ch = Chunks(m, 3, W).load(_ragged_clips(5))
    ref = ch.run(ragged=True)
    assert torch.isfinite(ref).all() and ref.abs().max() > 0
    assert torch.equal(ch.run(), ref)
    for i in range(3):
        assert torch.equal(ch.run(use_graph=True), ref), f"graph call {i}"


# ---- 3. the long form of both classes ----------------------------------------------------------------------------------------------------
CLASSES = {"score": PC, "regression": {}}


@pytest.mark.parametrize("kind", list(CLASSES))
@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_long_form_of_one_row_is_enhance(kind, precision):
    m, sampler = baseline(kind, precision), CLASSES[kind]
    for n in (20000, W):
        y = torch.from_numpy(_file(n, seed=n))
        ref = m.enhance(y, seed=5, **sampler) if kind == "score" else m.enhance(y)
        assert torch.isfinite(ref).all() and ref.abs().max() > 0
        out = long_form(m, y, seed=5, **sampler)
        assert out.shape == y.shape and out.device == y.device and torch.equal(out, ref), n
    assert torch.equal(long_form(m, y[None, None].cuda(), seed=5, **sampler), ref[None, None].cuda())


def _row_outputs(m, sampler, y, rows, seed):
    """Every row's output through the class's chunks call, ONE row per call, with the file's normalisation factor."""
    ch = Chunks(m, 1, W)
    nf = _normfac(y[None]).cpu().numpy()
    outs = []
    for r in rows:
        ch.load([y[r.start:r.start + r.length]], [seed], [r.frame0], nf)
        outs.append(ch.run(sampler or None, frame0=True, normfac=True)[0, :r.length].cpu().numpy())
    return outs


@pytest.mark.parametrize("kind,precision,n", [("score", "bf16", N4), ("score", "fp32", N3), ("regression", "bf16", N3), ("regression", "fp32", N4)])
def test_long_form_is_the_float32_stitch_of_its_rows(kind, precision, n):
    from flowdec_amd.longform import stitch_reference
    from flowdec_amd.noise import clip_seed
    m, sampler = baseline(kind, precision), CLASSES[kind]
    rows = _plan(n)
    assert len(rows) == (4 if n == N4 else 3)
    y = _file(n, seed=6)
    want = stitch_reference(_row_outputs(m, sampler, y, rows, clip_seed(9, 0)), rows, X)
    assert np.isfinite(want).all() and np.abs(want).max() > 0
    for rpc in (1, 2, 8):
        got = long_form(m, torch.from_numpy(y), seed=9, rows_per_call=rpc, **sampler)
        assert np.array_equal(got.numpy(), want), f"rows_per_call = {rpc}"
    assert np.array_equal(long_form(m, torch.from_numpy(y), seed=9, rows_per_call=2, use_graph=False, **sampler).numpy(), want)
    other = long_form(m, torch.from_numpy(y), seed=10, **sampler).numpy()
    assert np.array_equal(other, want) == (kind == "regression"), "another seed changes the score model's output (the regression model draws none)"
    # the two halves, over any split of the jobs
    call = m._chunks_call(**sampler)
    parts = torch.cat([m._enhance_long_rows(torch.from_numpy(y), call, jobs=j, seed=9, **GEO) for j in ((0, 1), (1, len(rows)))])
    assert np.array_equal(m._enhance_long_stitch(torch.from_numpy(y), parts, **GEO).numpy(), want)
    assert m._enhance_long_jobs(torch.from_numpy(y), **GEO) == len(rows)


@pytest.mark.parametrize("kind", list(CLASSES))
def test_long_form_two_channels_are_two_files_and_normfac(kind):
    m, sampler = baseline(kind, "bf16"), CLASSES[kind]
    y = torch.from_numpy(np.stack([_file(N3, seed=11), 3 * _file(N3, seed=12)]))[:, None]            # [2, 1, n], different levels
    both = long_form(m, y, seed=[21, 22], **sampler)
    assert both.shape == y.shape
    for c, s in enumerate((21, 22)):
        assert torch.equal(both[c, 0], long_form(m, y[c, 0], seed=[s], **sampler)), f"channel {c}"
    whole = long_form(m, y[0, 0], seed=[21], **sampler)
    causal = long_form(m, y[0, 0], seed=[21], normfac="causal", **sampler)
    fixed = long_form(m, y[0, 0], seed=[21], normfac=0.5, **sampler)
    assert all(torch.isfinite(x).all() and x.abs().max() > 0 for x in (causal, fixed))
    assert not torch.equal(fixed, whole) and not torch.equal(fixed, causal)
    assert torch.equal(long_form(m, y[0, 0], seed=[21], normfac=float(y[0, 0].abs().max()), **sampler), whole)
