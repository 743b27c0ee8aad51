"""GroupNorm statistics and the stand-alone passes at model shapes, and the two operators that are the drop-in boundary of the reference
(fd_upfirdn2d, fd_fused_bias_act), against plain NumPy references -- exactly where the data allows it.

fd_channel_sums on integers |x| <= 3: a 2048-pixel tile sums to |sum| <= 6144 and sum of squares <= 18432, integers below 2^15 at every
point of every summation order, so each float32 partial must EQUAL the integer reference of its tile.  fd_gn_finalize reduces such exact
partials in float64 (exact again: integers far below 2^53), so its affine pairs carry nothing but the float32 roundings of the last
few operations.  fd_upfirdn2d on integer data with kernel entries on a 1/4 grid is exact in float32 and in bf16.  The helpers used by the
sweep are checked on the CPU against the oracle in tests/test_fir_cpu.py."""
import os
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest
import torch

from conftest import rel_err
from oracle import flowdec_oracle as O
from test_hip_ops import REPORT

pytestmark = pytest.mark.gpu

DT = {"bf16": torch.bfloat16, "fp32": torch.float32}
U = 2.0 ** -24
TILE = 2048      # pixels per partial of fd_channel_sums


def report_line(line):
    os.makedirs(os.path.dirname(REPORT), exist_ok=True)
    with open(REPORT, "a") as f:
        f.write(line + "\n")


@pytest.fixture(scope="module")
def ops():
    from flowdec_amd import ops as _ops
    return _ops


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t if dtype is None else t.to(dtype)


# ---------------------------------------------------------------------------------------------------------
# fd_channel_sums, exact
# ---------------------------------------------------------------------------------------------------------
def tile_sums(x, tile):
    """x [B][H][W][C] integers -> int64 [B][tiles][C][2]: (sum, sum of squares) over consecutive runs of `tile` pixels of the H*W plane."""
    B, H, W, C = x.shape
    hw = H * W
    tiles = -(-hw // tile)
    v = np.zeros((B, tiles * tile, C), np.int32)
    v[:, :hw] = x.reshape(B, hw, C)
    v = v.reshape(B, tiles, tile, C)
    return np.stack([v.sum(axis=2, dtype=np.int64), (v * v).sum(axis=2, dtype=np.int64)], axis=-1)


SUM_SHAPES = [(768, 256), (384, 128), (488, 264), (24, 16), (64, 32), (683, 3)]     # 96 / 24 / 63 (ragged last) / 1 partial / exactly 2048 / 2049 pixels


@pytest.mark.parametrize("prec", ["bf16", "fp32"])
@pytest.mark.parametrize("C", [8, 16, 64, 256])
@pytest.mark.parametrize("H,W", SUM_SHAPES, ids=[f"{h}x{w}" for h, w in SUM_SHAPES])
def test_channel_sums_exact(ops, H, W, C, prec):
    from flowdec_amd import _lib as L
    B = 2
    rng = np.random.default_rng(zlib.crc32(f"sums/{H}/{W}/{C}/{prec}".encode()))
    x = rng.integers(-3, 4, (B, H, W, C), dtype=np.int8)
    want = tile_sums(x, TILE)
    assert np.abs(want[..., 0]).max() <= 6144 and want[..., 1].max() <= 18432          # the premise
    got = ops.channel_sums(dev(x).to(DT[prec]))
    torch.cuda.synchronize()
    tiles = L.load().fd_channel_sums_tiles(H, W)
    assert tiles == -(-(H * W) // TILE) and tuple(got.shape) == (B, tiles, C, 2)
    g = got.cpu().numpy().astype(np.float64)
    bad = int(np.count_nonzero(g != want))
    report_line(f"{'channel_sums_exact[' + f'{H}x{W},{C},{prec}' + ']':60s} tiles={tiles} mismatches={bad} tol=exact {'OK' if bad == 0 else 'FAIL'}")
    assert bad == 0, f"{bad} of {g.size} partial sums differ from the integer reference (max |diff| {np.abs(g - want).max():.1f})"


# ---------------------------------------------------------------------------------------------------------
# fd_gn_finalize on exact partials
# ---------------------------------------------------------------------------------------------------------
def gn_affine_f64(x, groups, gamma, beta, eps=1e-6):
    """float64 GroupNorm(groups, C) of x [B][H][W][C] as per-(b, c) pairs: y = a x + d.  Returns (a, d, mean * rstd * gamma)."""
    B, H, W, C = x.shape
    xg = x.reshape(B, H * W, groups, C // groups).astype(np.float64)
    mean = xg.mean(axis=(1, 3))
    var = ((xg - mean[:, None, :, None]) ** 2).mean(axis=(1, 3))
    rstd = np.repeat(1.0 / np.sqrt(var + eps), C // groups, axis=1)
    mean = np.repeat(mean, C // groups, axis=1)
    a = rstd * gamma.astype(np.float64)
    return a, beta.astype(np.float64) - mean * a, mean * a


def gn_params(rng, C):
    return (1 + 0.1 * rng.standard_normal(C)).astype(np.float32), (0.1 * rng.standard_normal(C)).astype(np.float32)


def conv_format_partials(ops, x, rng):
    """The partial sums of x in the layout the convolution epilogue emits (one partial per 16 x 16 tile, channel stride =
    fd_conv_cout_pad(C)), from the integer reference; the padding channels hold junk that fd_gn_finalize must not read."""
    from flowdec_amd import _lib as L
    B, H, W, C = x.shape
    lib = L.load()
    th, tw = -(-H // 16), -(-W // 16)
    assert lib.fd_conv_stats_tiles(H, W) == th * tw
    stride = lib.fd_conv_cout_pad(C)
    v = np.zeros((B, th * 16, tw * 16, C), np.int64)
    v[:, :H, :W] = x
    v = v.reshape(B, th, 16, tw, 16, C)
    part = np.full((B, th * tw, stride, 2), 1e6, np.float32)
    part[:, :, :C, 0] = v.sum(axis=(2, 4)).reshape(B, th * tw, C)
    part[:, :, :C, 1] = (v * v).sum(axis=(2, 4)).reshape(B, th * tw, C)
    return dev(part), stride


def assert_affine(name, x, aff, groups, gamma, beta, tol=2e-6):
    a, d, _ = gn_affine_f64(x, groups, gamma, beta)
    got = x.astype(np.float64) * aff[:, None, None, :, 0] + aff[:, None, None, :, 1]
    ref = x.astype(np.float64) * a[:, None, None, :] + d[:, None, None, :]
    e = rel_err(got, ref)
    report_line(f"{name:60s} err={e:.3e} tol={tol:.1e} {'OK' if e < tol else 'FAIL'}")
    assert e < tol, f"{name}: rel err {e:.3e} >= {tol:.1e}"


@pytest.mark.parametrize("prec", ["bf16", "fp32"])
@pytest.mark.parametrize("H,W,C", [(488, 264, 64), (768, 256, 256), (24, 16, 8)])
def test_gn_finalize_one_source(ops, H, W, C, prec):
    rng = np.random.default_rng(zlib.crc32(f"gn1/{H}/{W}/{C}/{prec}".encode()))
    x = rng.integers(-3, 4, (2, H, W, C), dtype=np.int8)
    gam, bet = gn_params(rng, C)
    part = ops.channel_sums(dev(x).to(DT[prec]))
    groups = min(C // 4, 32)
    aff = ops.gn_finalize(part, C, None, 0, dev(gam), dev(bet), groups, H * W).cpu().numpy()
    assert_affine(f"gn_finalize_exact_partials[{H}x{W},{C},{prec}]", x, aff, groups, gam, bet)


@pytest.mark.parametrize("prec", ["bf16", "fp32"])
@pytest.mark.parametrize("H,W,C0,C1", [(40, 24, 256, 64), (488, 264, 64, 16), (20, 36, 128, 256)])
def test_gn_finalize_two_sources_mixed_geometry(ops, H, W, C0, C1, prec):
    """GroupNorm over a virtual concat whose halves bring partials of different tile counts and strides: tensor 0 in the convolution
    epilogue's layout (16 x 16 tiles, stride fd_conv_cout_pad(C0)), tensor 1 from fd_channel_sums (2048-pixel tiles, stride C1).
    256 + 64 with 32 groups has 10 channels per group: group 25 (channels 250 .. 259) straddles the two tensors."""
    rng = np.random.default_rng(zlib.crc32(f"gn2/{H}/{W}/{C0}/{C1}/{prec}".encode()))
    C = C0 + C1
    x = rng.integers(-3, 4, (2, H, W, C), dtype=np.int8)
    x[..., C0:] += 2                                                     # the two tensors differ in mean: a straddling group sees both
    gam, bet = gn_params(rng, C)
    p0, stride0 = conv_format_partials(ops, x[..., :C0], rng)
    p1 = ops.channel_sums(dev(x[..., C0:]).to(DT[prec]))
    assert (p0.shape[1], stride0) != (p1.shape[1], C1)
    groups = min(C // 4, 32)
    assert (C0, C1) != (256, 64) or (C // groups == 10 and C0 % (C // groups) != 0)
    aff = ops.gn_finalize(p0, C0, p1, C1, dev(gam), dev(bet), groups, H * W).cpu().numpy()
    assert_affine(f"gn_finalize_mixed_sources[{H}x{W},{C0}+{C1},{prec}]", x, aff, groups, gam, bet)
    # ... and with the roles swapped (fd_channel_sums partials first)
    p0b = ops.channel_sums(dev(x[..., :C0]).to(DT[prec]))
    p1b, _ = conv_format_partials(ops, x[..., C0:], rng)
    aff2 = ops.gn_finalize(p0b, C0, p1b, C1, dev(gam), dev(bet), groups, H * W).cpu().numpy()
    assert np.array_equal(aff, aff2)                                     # the same exact sums reduced in float64: the same bits


@pytest.mark.parametrize("prec", ["bf16", "fp32"])
def test_gn_finalize_ill_conditioned(ops, prec):
    """x = 60 + integers in [-2, 2]: the mean is about 42 standard deviations, so SS/n - mean^2 = 3602 - 3600 cancels three digits.  What
    the float64 reduction of float32 partials can promise here: the partials are exact (sums <= 62 * 2048 < 2^17, sums of squares <=
    62^2 * 2048 < 2^23: integers below 2^24 in any order), their float64 totals are exact, and the cancellation costs float64 about
    3600 / 2 * 2^-52 = 4e-13 relative in the variance -- nothing at float32 scale.  So the pair (a, d) is the correctly computed float64
    pair up to its last float32 operations: rstd and mean * rstd rounded to float32, one product each with gamma, one subtraction:
        |a - a_ref| <= 2 u |a_ref|,   |d - d_ref| <= 2 u |mean rstd gamma| + u |d_ref|      (u = 2^-24; + 1e-11 relative for float64).
    NOT promised, and not asserted: 2e-6 on the normalised output y = a x + d.  |a x| and |d| are about 42 where |y| is about 1, so the
    float32 rounding of the pair alone is worth 42 * 3 u = 8e-6 of y; the exact statistics cannot change that."""
    rng = np.random.default_rng(5 if prec == "bf16" else 6)
    H, W, C = 488, 264, 64
    x = (60 + rng.integers(-2, 3, (2, H, W, C))).astype(np.int16)
    gam, bet = gn_params(rng, C)
    xd = dev(x.astype(np.float32)).to(DT[prec])
    assert torch.equal(xd.float().cpu(), torch.from_numpy(x.astype(np.float32)))      # exact in the storage type
    part = ops.channel_sums(xd)
    assert np.array_equal(part.cpu().numpy().astype(np.int64), tile_sums(x.astype(np.int32), TILE))
    groups = 16
    aff = ops.gn_finalize(part, C, None, 0, dev(gam), dev(bet), groups, H * W).cpu().numpy().astype(np.float64)
    a, d, mrg = gn_affine_f64(x, groups, gam, bet)
    ratio = float(np.abs(mrg / gam).min())
    assert ratio >= 30, ratio
    ea = np.abs(aff[..., 0] - a) / ((2 * U + 1e-11) * np.abs(a))
    ed = np.abs(aff[..., 1] - d) / ((2 * U + 1e-11) * np.abs(mrg) + U * np.abs(d))
    report_line(f"{'gn_finalize_ill_conditioned[' + prec + ']':60s} mean/std={ratio:.1f} worst/bound a={ea.max():.3f} d={ed.max():.3f} "
                f"{'OK' if max(ea.max(), ed.max()) <= 1 else 'FAIL'}")
    assert ea.max() <= 1.0 and ed.max() <= 1.0, (ea.max(), ed.max())


# ---------------------------------------------------------------------------------------------------------
# fd_gn_silu_apply at model size and beyond the grid cap
# ---------------------------------------------------------------------------------------------------------
def half_ulp_bf16(v):
    m, e = np.frexp(np.abs(v))
    return np.where(m == 0, 0.0, np.ldexp(1.0, e - 9))


@pytest.mark.parametrize("prec", ["bf16", "fp32"])
@pytest.mark.parametrize("B,H,W,C", [(8, 768, 256, 64), (3, 768, 256, 256)], ids=["8x768x256x64", "3x768x256x256_loops"])
def test_gn_silu_apply_elementwise_bound(ops, B, H, W, C, prec):
    """silu(a x + d) per element against float64 with the operand budget derived in tests/test_hip_fir.py (fmaf, __expf, 1 + e, rcp,
    multiply):  |got - s| <= E(t) u |s|,  E(t) = |1 + t (1 - sig)| + (1 - sig) (2 |t| + 2) + 4   [+ half a bf16 ulp for the store].
    3 x 768 x 256 x 256 is 18.9 M eight-channel vectors, above the grid cap of 2^16 workgroups x 256 threads: the kernel loops."""
    from test_hip_fir import act_operand
    rng = np.random.default_rng(zlib.crc32(f"apply/{B}/{C}/{prec}".encode()))
    assert (B * H * W * C // 8 > 65536 * 256) == (C == 256)
    g = torch.Generator(device="cuda").manual_seed(int(rng.integers(1 << 30)))
    x = (4 * torch.rand(B, H, W, C, device="cuda", generator=g) - 2).to(DT[prec])
    a = rng.uniform(0.75, 1.25, (B, C)).astype(np.float32)
    d = (2.0 * rng.integers(0, 2, (B, C)) + rng.uniform(-0.5, 0.5, (B, C))).astype(np.float32)
    out = ops.gn_silu_apply(x, dev(np.stack([a, d], -1)))
    torch.cuda.synchronize()
    xh, got = x.float().cpu().numpy(), out.float().cpu().numpy()

    def clip(b):
        s, budget = act_operand(xh[b], a[b], d[b])
        bound = (budget - 8.0) * U * np.abs(s)          # act_operand's budget includes the 8 fma of the FIR behind it
        if prec == "bf16":
            bound = bound + half_ulp_bf16(np.abs(s) + bound)
        err = np.abs(got[b].astype(np.float64) - s)
        ratio = np.divide(err, bound, out=np.where(err > 0, np.inf, 0.0), where=bound > 0)
        return float(ratio.max()), float((err ** 2).sum()), float((s ** 2).sum())

    with ThreadPoolExecutor(max_workers=min(8, B)) as ex:
        res = list(ex.map(clip, range(B)))
    worst = max(r[0] for r in res)
    e2 = float(np.sqrt(sum(r[1] for r in res) / sum(r[2] for r in res)))
    tol = 4e-3 if prec == "bf16" else 2e-6
    report_line(f"{'gn_silu_apply[' + f'{B}x{H}x{W}x{C},{prec}' + ']':60s} err={e2:.3e} tol={tol:.1e} worst/bound={worst:.3f} "
                f"{'OK' if worst <= 1 and e2 < tol else 'FAIL'}")
    assert e2 < tol and worst <= 1.0, (e2, worst)


# ---------------------------------------------------------------------------------------------------------
# fd_upfirdn2d: seeded sweep against a NumPy restatement of the operator
# ---------------------------------------------------------------------------------------------------------
def upfirdn2d_f64(x, k, up_x, up_y, down_x, down_y, pad_x0, pad_x1, pad_y0, pad_y1):
    """upfirdn2d on x [major][in_h][in_w][minor] in float64, step by step as the operator is defined: insert up - 1 zeros after every
    sample, pad with zeros (a negative pad crops instead), correlate with the flipped kernel over the valid positions, keep every
    down-th sample."""
    x = np.asarray(x, np.float64)
    major, h, w, minor = x.shape
    u = np.zeros((major, h * up_y, w * up_x, minor))
    u[:, ::up_y, ::up_x] = x
    u = np.pad(u, ((0, 0), (max(pad_y0, 0), max(pad_y1, 0)), (max(pad_x0, 0), max(pad_x1, 0)), (0, 0)))
    u = u[:, max(-pad_y0, 0):u.shape[1] - max(-pad_y1, 0), max(-pad_x0, 0):u.shape[2] - max(-pad_x1, 0)]
    kh, kw = k.shape
    oh, ow = u.shape[1] - kh + 1, u.shape[2] - kw + 1
    if oh <= 0 or ow <= 0:
        return np.zeros((major, 0, 0, minor))
    flipped = np.asarray(k, np.float64)[::-1, ::-1]
    out = np.zeros((major, oh, ow, minor))
    for i in range(kh):
        for j in range(kw):
            out += flipped[i, j] * u[:, i:i + oh, j:j + ow]
    return out[:, ::down_y, ::down_x]


UPFIRDN_DRAWS = 40


def upfirdn_draw(i):
    """Draw i of the sweep: (x int-valued float64 [major][h][w][minor] in [-3, 3], kernel on a 1/4 grid in [-1, 1], the 8 arguments
    (up_x, up_y, down_x, down_y, pad_x0, pad_x1, pad_y0, pad_y1)).  <= 20 taps x 3 x 1: |result| <= 60 on a 1/4 grid -- 8 bits."""
    rng = np.random.default_rng(1000 + i)
    kh, kw = ((1, 1), (4, 5), (4, 1), (1, 5))[i] if i < 4 else (int(rng.integers(1, 5)), int(rng.integers(1, 6)))
    major, minor = int(rng.integers(1, 10)), int(rng.integers(1, 10))
    h, w = int(rng.integers(2, 12)), int(rng.integers(2, 12))
    ups, downs = rng.integers(1, 4, 2), rng.integers(1, 4, 2)
    while True:
        pads = rng.integers(-2, 4, 4)
        if h * ups[1] + pads[2] + pads[3] >= kh and w * ups[0] + pads[0] + pads[1] >= kw:
            break
    x = rng.integers(-3, 4, (major, h, w, minor)).astype(np.float64)
    k = rng.integers(-4, 5, (kh, kw)) / 4.0
    return x, k, tuple(int(v) for v in (ups[0], ups[1], downs[0], downs[1], pads[0], pads[1], pads[2], pads[3]))


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_upfirdn2d_sweep_exact(ops, prec):
    from flowdec_amd import _lib as L
    lib = L.load()
    for i in range(UPFIRDN_DRAWS):
        x, k, args = upfirdn_draw(i)
        ref = upfirdn2d_f64(x, k, *args)
        up_x, up_y, down_x, down_y, px0, px1, py0, py1 = args
        assert ref.shape[1] == lib.fd_upfirdn2d_out_size(x.shape[1], up_y, down_y, py0, py1, k.shape[0]), (i, args)
        assert ref.shape[2] == lib.fd_upfirdn2d_out_size(x.shape[2], up_x, down_x, px0, px1, k.shape[1]), (i, args)
        out = ops.upfirdn2d_raw(dev(x.astype(np.float32)).to(DT[prec]), dev(k.astype(np.float32)), *args)
        got = out.float().cpu().numpy().astype(np.float64)
        assert got.shape == ref.shape, (i, args, got.shape, ref.shape)
        bad = int(np.count_nonzero(got != ref))
        report_line(f"{'upfirdn2d_sweep[' + str(i) + ',' + prec + ']':60s} x={x.shape} k={k.shape} up/down/pads={args} mismatches={bad} tol=exact "
                    f"{'OK' if bad == 0 else 'FAIL'}")
        assert bad == 0, f"draw {i} {args} kernel {k.shape} x {x.shape}: {bad} of {got.size} outputs differ (max |diff| {np.abs(got - ref).max():.3e})"


# ---------------------------------------------------------------------------------------------------------
# fd_fused_bias_act
# ---------------------------------------------------------------------------------------------------------
# name, shape, axis of the bias (None = no bias), act, alpha, scale
BIAS_ACT_CASES = [
    ("lrelu_mid_axis", (4, 6, 5), 1, 3, 0.2, float(np.sqrt(2.0))),
    ("lrelu_last_axis", (7, 33, 13), 2, 3, 0.01, 0.5),             # n = 3003, not a multiple of 256
    ("linear_mid_axis", (3, 5, 70), 1, 1, 0.2, 1.5),               # act 1 ignores alpha
    ("linear_last_axis", (2, 9, 257), 2, 1, 0.0, 1.0),
    ("lrelu_no_bias", (1001,), None, 3, 0.3, 2.0),
    ("linear_no_bias", (255,), None, 1, 0.2, -1.0),
    ("lrelu_first_axis", (5, 300), 0, 3, 0.2, 1.0),
]


@pytest.mark.parametrize("case", BIAS_ACT_CASES, ids=[c[0] for c in BIAS_ACT_CASES])
def test_fused_bias_act_formula(case):
    """out = scale * act(x + bias[(i / step_b) % size_b]), act 1 = identity, act 3 = leaky ReLU with slope alpha."""
    from flowdec_amd import _lib as L
    name, shape, axis, act, alpha, scale = case
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    x = rng.standard_normal(shape).astype(np.float32)
    n = x.size
    v = x.astype(np.float64)
    bias = None
    step_b = size_b = 0
    if axis is not None:
        size_b = shape[axis]
        step_b = int(np.prod(shape[axis + 1:], dtype=np.int64))
        bias = rng.standard_normal(size_b).astype(np.float32)
        v = v + bias.astype(np.float64).reshape([-1 if i == axis else 1 for i in range(len(shape))])
    ref = (np.where(v > 0, v, v * np.float64(np.float32(alpha))) if act == 3 else v) * np.float64(np.float32(scale))
    xd, bd = dev(x), (None if bias is None else dev(bias))
    out = torch.full_like(xd, float("nan"))
    L.check(L.load().fd_fused_bias_act(L.ptr(xd), L.ptr(bd), L.ptr(out), n, step_b, size_b, act, alpha, scale, L.stream()))
    got = out.cpu().numpy().astype(np.float64)
    e = rel_err(got, ref)
    worst = float(np.abs(got - ref).max() / np.abs(ref).max())
    report_line(f"{'fused_bias_act[' + name + ']':60s} err={e:.3e} tol=1.0e-06 {'OK' if e < 1e-6 else 'FAIL'}")
    assert e < 1e-6 and worst < 1e-6, (e, worst)
    assert np.all(np.abs(got - ref) <= 1e-6 * np.abs(ref) + 1e-12)
