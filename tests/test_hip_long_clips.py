"""Clips longer than ~43 s: images whose activation tensors exceed 2 GiB (bf16) / 4 GiB (f32 storage) and, at 90 s, 2^31 elements.

The conv kernels address a workgroup's input from the first row of its halo band (64-bit base) with 32-bit per-lane offsets inside the
band.  Operator level: a large launch must give, row for row, exactly what the same call gives on a small cut-out of the rows around
a band (first rows, rows straddling 2^31 / 2^32 bytes, last rows) -- the per-pixel arithmetic of a kernel does not depend on where the
image lies in memory.  The direct and head kernels, fed the small-integer data of test_hip_conv_exact.py, must also EQUAL a float64
convolution of each band.  Model level: 45 / 60 / 90 s clips through the full-width 75m model."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_hip_model import TOL_WAVE_FULL, _cache, check, make_model, tol_wave_full

pytestmark = pytest.mark.gpu

H, W = 768, 11264      # the top level of a 90 s clip: T_pad = 11264
MARGIN = 16            # cut-out rows on each side of a band (a multiple of 16 keeps the 16-row tiling of every kernel)


@pytest.fixture(scope="module")
def ops():
    from flowdec_amd import ops as _ops
    return _ops


def counted(ops, fn):
    before = ops.conv_kernel_counts()
    out = fn()
    torch.cuda.synchronize()
    after = ops.conv_kernel_counts()
    return out, {k: after[k] - before[k] for k in after if after[k] != before[k]}


def bands(row_bytes, limits):
    """Output row bands [o0, o1): the first rows, the rows that straddle each byte limit, the last rows."""
    out = [(0, 16)]
    for lim in limits:
        r = lim // row_bytes
        assert 0 < r < H - 16, "the image must straddle the limit"
        out.append((r // 16 * 16, r // 16 * 16 + 32))
    return out + [(H - 16, H)]


def cut(t, i0, i1):
    return None if t is None else t[:, i0:i1].contiguous()


def gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def rand_img(C, dtype, g, exact):
    if exact:   # small integers: exact in bf16 and f32
        return torch.randint(-2, 3, (1, H, W, C), generator=g, device="cuda", dtype=torch.int8).to(dtype)
    return torch.randn(1, H, W, C, generator=g, device="cuda", dtype=dtype)


def rand_w(Cout, Cin, k, g, exact):
    if exact:   # multiples of 1/4, |w| <= 1/2
        return torch.randint(-2, 3, (Cout, Cin, k, k), generator=g, device="cuda").float() / 4
    return torch.randn(Cout, Cin, k, k, generator=g, device="cuda") / (3 * Cin ** 0.5)


def ref_f64(x, w, bias, o0, o1, cols=None):
    """float64 convolution (CPU) of output rows [o0, o1) and columns `cols` (zero padding); x NHWC on the device, w [Cout, Cin, k, k]."""
    p = w.shape[-1] // 2
    c0, c1 = (0, W) if cols is None else cols
    i0, i1, j0, j1 = max(o0 - p, 0), min(o1 + p, H), max(c0 - p, 0), min(c1 + p, W)
    xc = x[:, i0:i1, j0:j1].double().cpu().permute(0, 3, 1, 2)
    xc = F.pad(xc, (p - (c0 - j0), p - (j1 - c1), p - (o0 - i0), p - (i1 - o1)))
    return F.conv2d(xc, w.double().cpu(), None if bias is None else bias.double().cpu()).permute(0, 2, 3, 1)


def stats_rows(st, r0, r1):
    """GroupNorm partials [B, tiles, CoutPad, 2] of the 16-row tile rows covering image rows [r0, r1)."""
    B, _, cp, _ = st.shape
    return st.reshape(B, -1, (W + 15) // 16, cp, 2)[:, r0 // 16:r1 // 16]


def run_case(ops, name, Cin, Cout, dtype, winograd, expect, exact=False, ksize=3, operands=False, concat=False, shortcut=False,
             affine=False, skip=False, stats=False, tile_bn=0, seed=0):
    g = gen(seed)
    esize = 2 if dtype == torch.bfloat16 else 4
    x0 = rand_img(Cin, dtype, g, exact)
    x1 = rand_img(Cin, dtype, g, exact) if concat else None
    sc0 = rand_img(Cin, dtype, g, exact) if shortcut else None
    sk = rand_img(Cout, dtype, g, exact) if skip else None
    Ctot = Cin * (2 if concat else 1)
    w = rand_w(Cout, Ctot, ksize, g, exact)
    w_sc = rand_w(Cout, Cin, 1, g, exact) if shortcut else None
    bias = (torch.randint(-4, 5, (Cout,), generator=g, device="cuda").float() / 4) if exact else torch.randn(Cout, generator=g, device="cuda")
    aff = None
    if affine:
        aff = torch.stack([0.5 + 0.5 * torch.rand(1, Ctot, generator=g, device="cuda"), 0.2 * torch.randn(1, Ctot, generator=g, device="cuda")], -1).contiguous()
    scale = 1.0 if exact else 2 ** -0.5
    pw = ops.pack_conv_weight(w, C0=Cin, dtype=dtype, w_sc=w_sc, winograd=winograd, bf16_operands=operands)

    def call(a0, a1, s0, skp):
        return ops.conv2d(a0, pw, Cout, ksize, x1=a1, affine=aff, bias=bias, skip=skp, scale=scale, sc0=s0, want_stats=stats,
                          winograd=winograd, tile_bn=tile_bn, bf16_operands=operands)
    big, kc = counted(ops, lambda: call(x0, x1, sc0, sk))
    assert kc == {expect: 1}, (name, kc)
    big, big_st = big if stats else (big, None)
    assert torch.isfinite(big.float()[:, ::64]).all()
    largest = max(Cin, Cout) * W * esize   # the bytes of one row of the widest single tensor
    limits = [1 << 31] + ([1 << 32] if esize == 4 else [])
    for o0, o1 in bands(largest, limits):
        i0, i1 = max(o0 - MARGIN, 0), min(o1 + MARGIN, H)
        small, kc = counted(ops, lambda: call(cut(x0, i0, i1), cut(x1, i0, i1), cut(sc0, i0, i1), cut(sk, i0, i1)))
        assert kc == {expect: 1}, (name, kc)
        small, small_st = small if stats else (small, None)
        assert torch.equal(big[:, o0:o1], small[:, o0 - i0:o1 - i0]), f"{name}: rows {o0}..{o1} differ from the cut-out launch"
        if stats:   # per-tile partial sums depend on the tile's outputs only
            assert torch.equal(stats_rows(big_st, o0, o1), stats_rows(small_st, o0 - i0, o1 - i0)), f"{name}: statistics of rows {o0}..{o1} differ"
        if exact:   # the direct / head kernels: the exact value, one rounding at the store
            cols = None if Cout == 4 or ksize == 1 else (W - 2048, W)
            ref = ref_f64(x0, w, bias, o0, o1, cols)
            got = big[:, o0:o1] if cols is None else big[:, o0:o1, cols[0]:cols[1]]
            assert torch.equal(got.cpu(), ref.float().to(dtype)), f"{name}: rows {o0}..{o1} differ from the float64 convolution"
    del big, x0, x1, sc0, sk
    torch.cuda.empty_cache()


def test_wino4_bf16_resblock_conv1(ops):
    """F(4,3) bf16, 256 -> 256: GroupNorm+SiLU operand transform, folded 1x1 shortcut, bias, 1/sqrt(2), statistics (Conv_1 + Conv_2)."""
    run_case(ops, "wino4 conv1", 256, 256, torch.bfloat16, 4, "WINO4", affine=True, shortcut=True, stats=True, seed=1)


def test_wino4_bf16_concat_skip(ops):
    """F(4,3) bf16 over two 256-channel concat segments, with a residual input."""
    run_case(ops, "wino4 concat", 256, 256, torch.bfloat16, 4, "WINO4", concat=True, affine=True, skip=True, seed=2)


def test_wino_f23_bf16(ops):
    """F(2,3) bf16 (conv_wino.hip: every 3x3 conv under conv_algo='winograd'), 256 -> 256 with GroupNorm+SiLU, residual, statistics."""
    run_case(ops, "wino f23", 256, 256, torch.bfloat16, True, "WINO", affine=True, skip=True, stats=True, seed=9)


def test_wino44f(ops):
    """2-D F(4x4, 3x3) in float32, 256 -> 256 with GroupNorm+SiLU and a residual input."""
    run_case(ops, "wino44f", 256, 256, torch.float32, 44, "WINO44F", affine=True, skip=True, stats=True, seed=3)


def test_wino4f_explicit(ops):
    """F(4,3) in float32 (winograd=4 with f32 storage), with the folded shortcut."""
    run_case(ops, "wino4f", 256, 256, torch.float32, 4, "WINO4F", affine=True, shortcut=True, seed=4)


def test_direct_f32_bf16x3(ops):
    """Direct kernel, f32 storage, split-bf16 operands, 128 -> 128 (4.4 GB per image: past the old 4 GiB limit)."""
    run_case(ops, "direct bf16x3", 128, 128, torch.float32, False, "DIRECT_SPLIT", exact=True, operands="x3", seed=5)


def test_direct_f32_bf16_operands(ops):
    """Direct kernel, f32 storage, bf16 operands (FD_BF16_OPERANDS), 128 -> 128."""
    run_case(ops, "direct mixed", 128, 128, torch.float32, False, "DIRECT_MIXED", exact=True, operands=True, seed=10)


def test_direct_bf16_persist(ops):
    """Direct kernel, bf16, persistent register-epilogue configuration (FD_TILE_PERSIST: the loader moves across tiles), 256 -> 256,
    with the statistics written through their buffer resource."""
    run_case(ops, "direct persist", 256, 256, torch.bfloat16, False, "DIRECT", exact=True, stats=True, tile_bn="persist", seed=11)


def test_direct_bf16_chunk_ring(ops):
    """Direct kernel, bf16, low-latency chunk-ring configuration (64 couts per workgroup), 256 -> 64, with statistics."""
    run_case(ops, "direct chunk ring", 256, 64, torch.bfloat16, False, "DIRECT", exact=True, stats=True, tile_bn="64c", seed=12)


def test_direct_bf16_1x1(ops):
    """Direct kernel, bf16, 1x1, 256 -> 256."""
    run_case(ops, "direct 1x1", 256, 256, torch.bfloat16, False, "DIRECT", exact=True, ksize=1, seed=6)


def test_head_bf16(ops):
    """Pyramid head C -> 4, bf16 (conv_head.hip: want_stats=False)."""
    run_case(ops, "head", 256, 4, torch.bfloat16, False, "HEAD", exact=True, seed=7)


def test_headf_f32(ops):
    """Pyramid head C -> 4, float32 (conv_headf.hip)."""
    run_case(ops, "headf", 256, 4, torch.float32, False, "HEADF", exact=True, seed=8)


# ---------------------------------------------------------------------------------------------------------
# whole model, full width (75m)
def clip_and_noise(seconds, seed, B=1):
    from flowdec_amd import _lib as L_
    lib = L_.load()
    L = int(seconds * 48000)
    Tp = lib.fd_padded_frames(lib.fd_num_frames(L, 384))
    g = gen(seed)
    y = 0.1 * torch.randn(B, 1, L, device="cuda", generator=g)
    nz = torch.randn(B, 1, 768, Tp, dtype=torch.complex64, device="cuda", generator=g)
    return y, nz, L, Tp


def free_models():
    _cache.clear()
    torch.cuda.empty_cache()


def test_60s_clip_all_modes():
    """A 60 s clip (T_pad = 7552: 3.0 GB per bf16 activation, 5.9 GB in f32) in bf16, bf16x3, fp32 and bf16 with conv_algo='winograd'
    (F(2,3) kernel): finite, non-zero, and the modes agree to their tolerances over the whole clip and over its last two seconds (the
    highest addresses)."""
    free_models()
    y, nz, L, Tp = clip_and_noise(60, 5)
    assert Tp == 7552
    outs = {}
    for prec in ("bf16", "bf16x3", "fp32", "bf16 f23"):
        if prec == "bf16 f23":   # conv_algo='winograd': F(2,3) at every 3x3 conv, the top level included
            import flowdec_amd
            from oracle import flowdec_oracle as O
            m = flowdec_amd.from_preset("flowdec_75m", precision="bf16", nf=64, conv_algo="winograd")
            m.load_state_dict({k: torch.from_numpy(v) for k, v in O.random_state_dict(seed=64, nf=64).items()}, strict=False)
            m = m.cuda()
        else:
            m = make_model(64, 64, prec)
        outs[prec] = m.enhance(y, N=1, solver="euler", noise=nz).cpu().numpy()
        assert np.isfinite(outs[prec]).all() and np.abs(outs[prec]).max() > 0
        del m
        free_models()      # the f32 workspaces are tens of GB
    tail = slice(L - 2 * 48000, L)
    check("clip60[bf16x3 vs fp32]", outs["bf16x3"], outs["fp32"], TOL_WAVE_FULL["bf16x3"])
    check("clip60_tail[bf16x3 vs fp32]", outs["bf16x3"][..., tail], outs["fp32"][..., tail], TOL_WAVE_FULL["bf16x3"])
    check("clip60[bf16 vs fp32]", outs["bf16"], outs["fp32"], tol_wave_full("bf16", "euler_N6"))
    check("clip60_tail[bf16 vs fp32]", outs["bf16"][..., tail], outs["fp32"][..., tail], tol_wave_full("bf16", "euler_N6"))
    check("clip60[bf16 F(2,3) vs fp32]", outs["bf16 f23"], outs["fp32"], tol_wave_full("bf16", "euler_N6"))
    check("clip60_tail[bf16 F(2,3) vs fp32]", outs["bf16 f23"][..., tail], outs["fp32"][..., tail], tol_wave_full("bf16", "euler_N6"))


def test_batch_offset_past_4gib():
    """Two 45 s clips in one bf16 call: clip 1 starts 3.3 GB into every activation tensor and must equal the clip enhanced alone, bit
    for bit -- through enhance (one [B] call) and through enhance_batch (ragged)."""
    free_models()
    y, nz, L, Tp = clip_and_noise(45, 6, B=2)
    m = make_model(64, 64, "bf16")
    two = m.enhance(y, N=1, solver="euler", noise=nz)
    one = m.enhance(y[1:], N=1, solver="euler", noise=nz[1:])
    assert torch.isfinite(one).all() and float(one.abs().max()) > 0
    assert torch.equal(two[1:], one)
    del two
    rag = m.enhance_batch([y[0, 0], y[1, 0, :L - 4800]], N=1, solver="euler", noise=[nz[0], nz[1]])
    alone = m.enhance_batch([y[1, 0, :L - 4800]], N=1, solver="euler", noise=[nz[1]])
    assert torch.equal(rag[1], alone[0])
    del m
    free_models()


def test_90s_clip_bf16():
    """A 90 s clip in bf16 (T_pad = 11264: 2.2 G elements per activation tensor, beyond 2^31): finite; a second call and the eager
    path (use_graph=False) are bit-identical to the first graph replay."""
    free_models()
    y, nz, L, Tp = clip_and_noise(90, 7)
    assert Tp == 11264 and 768 * Tp * 256 > 2 ** 31
    m = make_model(64, 64, "bf16")
    a = m.enhance(y, N=1, solver="euler", noise=nz)
    assert torch.isfinite(a).all() and float(a.abs().max()) > 0
    b = m.enhance(y, N=1, solver="euler", noise=nz)
    assert torch.equal(a, b)
    c = m.enhance(y, N=1, solver="euler", noise=nz, use_graph=False)
    assert torch.equal(a, c)
    del m
    free_models()


def test_cli_max_seconds(tmp_path):
    """A 35 s file is skipped by default (the reference's 30 s rule) and enhanced with --max-seconds 40."""
    from flowdec_amd import enhance_cli
    from test_cli import synthetic_ckpt
    torch.save(synthetic_ckpt(), tmp_path / "m.ckpt")
    ind = tmp_path / "in"
    ind.mkdir()
    rng = np.random.default_rng(0)
    enhance_cli.save_wav(str(ind / "long.wav"), torch.from_numpy((0.1 * rng.standard_normal(35 * 48000)).astype(np.float32))[None], 48000)
    base = ["--ckpt", str(tmp_path / "m.ckpt"), "--files", str(ind), "--N", "1", "--solver", "euler"]
    res = enhance_cli.run(base + ["--outdir", str(tmp_path / "o1")])
    assert (res.n_done, res.n_too_long, res.exit_code) == (0, 1, 0)
    res = enhance_cli.run(base + ["--outdir", str(tmp_path / "o2"), "--max-seconds", "40"])
    assert (res.n_done, res.n_too_long, res.exit_code) == (1, 0, 0)
    x, sr = enhance_cli.load_wav(str(tmp_path / "o2" / "long.wav"))
    assert x.shape[-1] == 35 * 48000 and torch.isfinite(x).all()
