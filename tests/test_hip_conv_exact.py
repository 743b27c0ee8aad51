"""Exact-arithmetic parity of the direct and pyramid-head convolution kernels (conv_mfma.hip, conv_head.hip, conv_headf.hip).

With small-integer activations (|x| <= 2), weights on a 1/4 grid (|w| <= 1/2), biases on a 1/4 grid, integer residual inputs and scale 1
or 1/2, every product and every partial sum of a convolution is a multiple of 1/4 below 9 * 512 + shortcut + bias + skip in magnitude:
about 15 significant bits, well inside f32's 24.  Whatever the summation order and whatever the internal accumulation width of the
matrix cores, the float32 result must then EQUAL the float64 convolution, and the bf16 result must equal it after the one rounding of
the store.  A dropped tap, channel, pixel, chunk or bias row changes some output by at least 1/8 and fails the comparison however few
outputs it touches -- which the relative-L2 tolerances of test_hip_ops.py (6e-3 / 4e-4 / 2e-5 on random data) cannot promise.  Integers
of this size are exact in bf16, so the same data also pins the bf16-operand modes of float32 storage (FD_BF16_OPERANDS, and
FD_BF16X3_OPERANDS, whose lo halves are zero here).  The Winograd kernels are out of scope HERE: their weight transform divides by 6 and
24, which is exact only for weights on a 24 * 2^-k grid -- tests/test_hip_wino_exact.py covers them on such data.

Every launch is attributed to its kernel through fd_conv_kernel_counts (ops.conv_kernel_counts), against `expected_kernel`, a mirror of
the dispatch rule of fd_conv2d: if a change to the rule moves a case to another kernel, the case fails."""
import os
import zlib

import numpy as np
import pytest
import torch

from conftest import ROOT, rel_err
from oracle import flowdec_oracle as O
from test_hip_ops import CONV_CASES, REPORT

pytestmark = pytest.mark.gpu

DT = {"bf16": torch.bfloat16, "fp32": torch.float32}


@pytest.fixture(scope="module")
def ops():
    from flowdec_amd import ops as _ops
    return _ops


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t if dtype is None else t.to(dtype)


def nhwc(a_nchw, dtype):
    return dev(np.transpose(a_nchw, (0, 2, 3, 1)), dtype)


def from_nhwc(t):
    return np.transpose(t.float().cpu().numpy(), (0, 3, 1, 2))


def bf16r(a):
    return O.round_bf16(np.asarray(a, np.float32))


def report_line(line):
    os.makedirs(os.path.dirname(REPORT), exist_ok=True)
    with open(REPORT, "a") as f:
        f.write(line + "\n")


# ---------------------------------------------------------------------------------------------------------
# dispatch mirror and kernel counters
# ---------------------------------------------------------------------------------------------------------
HEAD_CK = {"bf16": 32, "fp32": 16}             # input channels per K chunk of conv_head.hip / conv_headf.hip
HEAD_MAX_CHUNKS = {"bf16": 16, "fp32": 32}     # MAX_STEPS / 9 of either kernel: the weights of 512 input channels in LDS


def expected_kernel(prec, C0, C1, Cout=4, k=3, stats=False, tile=0, shortcut=False, operands=False):
    """The kernel fd_conv2d launches for a non-Winograd call (conv_mfma.hip, the dispatch at the end of fd_conv2d, with
    fd_head_supported / fd_headf_supported).  prec = storage type; operands = the bf16_operands argument of ops.conv2d."""
    if operands is True:
        return "DIRECT_MIXED"
    if operands == "x3":
        return "DIRECT_SPLIT"
    ck = HEAD_CK[prec]
    chunks = -(-C0 // ck) + -(-C1 // ck)
    head = (Cout == 4 and k == 3 and not stats and not shortcut and chunks % 2 == 0 and chunks <= HEAD_MAX_CHUNKS[prec]
            and C0 % 4 == 0 and C1 % 4 == 0)
    # bf16: any call without a workgroup-width hint (FD_TILE_PERSIST is not one); fp32: no FD_TILE_* flag at all
    head = head and (tile in (0, "persist") if prec == "bf16" else tile == 0)
    if head:
        return "HEAD" if prec == "bf16" else "HEADF"
    return "DIRECT"


def counted(ops, fn):
    """Run fn(), return (its result, per-kernel change of the fd_conv2d dispatch counters)."""
    before = ops.conv_kernel_counts()
    out = fn()
    torch.cuda.synchronize()
    after = ops.conv_kernel_counts()
    return out, {k: after[k] - before[k] for k in after}


def assert_launched(delta, kernel, n, name):
    moved = {k: v for k, v in delta.items() if v}
    assert moved == {kernel: n}, f"{name}: expected {n} launch(es) of {kernel}, the dispatch counters moved by {moved}"


def test_expected_kernel_mirror_examples():
    """The mirror itself on the boundaries it encodes (independent of the GPU data below)."""
    assert expected_kernel("bf16", 64, 0) == "HEAD" and expected_kernel("fp32", 64, 0) == "HEADF"
    assert expected_kernel("bf16", 96, 0) == "DIRECT" and expected_kernel("fp32", 80, 0) == "DIRECT"        # odd chunk counts
    assert expected_kernel("bf16", 40, 0) == "HEAD" and expected_kernel("fp32", 40, 0) == "DIRECT"          # 2 vs 3 chunks
    assert expected_kernel("bf16", 512, 0) == "HEAD" and expected_kernel("bf16", 576, 0) == "DIRECT"       # the 512-channel limit
    assert expected_kernel("fp32", 256, 256) == "HEADF" and expected_kernel("fp32", 576, 0) == "DIRECT"
    assert expected_kernel("bf16", 64, 0, stats=True) == "DIRECT" and expected_kernel("bf16", 64, 0, tile=32) == "DIRECT"
    assert expected_kernel("bf16", 64, 0, tile="persist") == "HEAD" and expected_kernel("fp32", 64, 0, tile="persist") == "DIRECT"
    assert expected_kernel("bf16", 64, 0, Cout=8) == "DIRECT" and expected_kernel("fp32", 64, 0, k=1) == "DIRECT"
    assert expected_kernel("fp32", 64, 0, operands="x3") == "DIRECT_SPLIT" and expected_kernel("fp32", 64, 0, operands=True) == "DIRECT_MIXED"


# ---------------------------------------------------------------------------------------------------------
# exact-data runs of one fd_conv2d call
# ---------------------------------------------------------------------------------------------------------
def run_exact(ops, name, prec, B, H, W, C0, C1, Cout, k, bias_rows, use_skip, scale, S0=0, S1=0, tile=0, operands=False, stats=False):
    """One fd_conv2d call on exact data (module docstring), affine off; asserts the bit-exact result and returns the kernel it ran."""
    rng = np.random.default_rng(zlib.crc32(f"{name}/{prec}/{operands}/{tile}".encode()))
    storage = DT["bf16" if prec == "bf16" else "fp32"]
    Cin = C0 + C1
    x = rng.integers(-2, 3, (B, Cin, H, W)).astype(np.float64)
    w = rng.integers(-2, 3, (Cout, Cin, k, k)) / 4.0
    ref = O.conv2d(x, w, None)
    sc0 = sc1 = w_sc = None
    if S0:
        xs = rng.integers(-2, 3, (B, S0 + S1, H, W)).astype(np.float64)
        ws = rng.integers(-2, 3, (Cout, S0 + S1, 1, 1)) / 4.0
        ref = ref + O.conv2d(xs, ws, None)
        sc0 = nhwc(xs[:, :S0].astype(np.float32), storage)
        sc1 = nhwc(xs[:, S0:].astype(np.float32), storage) if S1 else None
        w_sc = dev(ws.astype(np.float32))
    bias = None
    if bias_rows:
        bv = rng.integers(-8, 9, (bias_rows, Cout)) / 4.0
        ref = ref + bv[:, :, None, None]
        bias = dev((bv if bias_rows > 1 else bv[0]).astype(np.float32))
    skip = None
    if use_skip:
        sk = rng.integers(-4, 5, (B, Cout, H, W)).astype(np.float64)
        ref = ref + sk
        skip = nhwc(sk.astype(np.float32), storage)
    ref = ref * scale
    assert np.array_equal(ref.astype(np.float32).astype(np.float64), ref)    # the premise: exact in f32
    x0 = nhwc(x[:, :C0].astype(np.float32), storage)
    x1 = nhwc(x[:, C0:].astype(np.float32), storage) if C1 else None
    pw = ops.pack_conv_weight(dev(w.astype(np.float32)), C0=C0, dtype=storage, w_sc=w_sc, S0=S0 if S0 else None, bf16_operands=operands)
    res, delta = counted(ops, lambda: ops.conv2d(x0, pw, Cout, k, x1=x1, bias=bias, skip=skip, scale=scale, sc0=sc0, sc1=sc1,
                                                 want_stats=stats, tile_bn=tile, bf16_operands=operands))
    got = from_nhwc(res[0] if stats else res).astype(np.float64)
    want = bf16r(ref).astype(np.float64) if prec == "bf16" else ref
    kernel = expected_kernel(prec, C0, C1, Cout, k, stats, tile, bool(S0), operands)
    bad = int(np.count_nonzero(got != want))
    report_line(f"{'conv_exact[' + name + ',' + prec + (',' + str(operands) if operands else '') + ']':60s} "
                f"mismatches={bad} maxdiff={float(np.abs(got - want).max()):.3e} tol=exact kernel={kernel}+{delta.get(kernel, 0)} "
                f"{'OK' if bad == 0 else 'FAIL'}")
    assert bad == 0, f"{name}[{prec}]: {bad} of {got.size} outputs differ from the exact result (max |diff| {np.abs(got - want).max():.3e})"
    assert_launched(delta, kernel, 1, name)
    return kernel


# (a) head kernels, ACT = false.  name, precisions, B, H, W, C0, C1, bias_rows ("B" = one row per image), skip, scale.
# grids (blocks = B * ceil(H/16) * ceil(W/16)): 1, 3 (< 8: the XCD remap's short tail), 6, 9, 15, 18, 45 and 54 (not multiples of 8)
HEAD_CASES = [
    ("c64_1blk", ("bf16", "fp32"), 1, 16, 16, 64, 0, 1, False, 1.0),
    ("c128_3blk", ("bf16", "fp32"), 3, 16, 16, 128, 0, "B", True, 0.5),
    ("c256_45blk", ("bf16", "fp32"), 3, 48, 80, 256, 0, 1, True, 1.0),
    ("c256_b9_54blk", ("bf16", "fp32"), 9, 20, 36, 256, 0, "B", True, 0.5),
    ("c512_lds_limit", ("bf16", "fp32"), 1, 20, 36, 512, 0, 0, True, 0.5),
    ("c24_partial", ("fp32",), 9, 1, 16, 24, 0, "B", False, 1.0),            # chunks 16 + 8
    ("c56_partial", ("bf16", "fp32"), 1, 24, 8, 56, 0, 1, True, 1.0),       # bf16 32 + 24, fp32 16 + 16 + 16 + 8
    ("c40_partial", ("bf16",), 3, 20, 36, 40, 0, 0, True, 0.5),              # chunks 32 + 8
    ("cat8_8", ("bf16", "fp32"), 9, 24, 8, 8, 8, "B", True, 1.0),           # two partial chunks, one per segment
    ("cat64_64", ("bf16", "fp32"), 1, 20, 36, 64, 64, 1, False, 1.0),
    ("cat96_32", ("bf16", "fp32"), 3, 16, 16, 96, 32, "B", True, 0.5),
    ("cat72_8", ("bf16", "fp32"), 1, 48, 80, 72, 8, 0, False, 1.0),
    ("cat256_256", ("bf16", "fp32"), 3, 24, 8, 256, 256, 1, True, 1.0),     # the 512-channel limit over two segments
    ("c128_row_1x16", ("bf16", "fp32"), 1, 1, 16, 128, 0, 1, True, 0.5),
]


@pytest.mark.parametrize("prec,case", [(p, c) for c in HEAD_CASES for p in c[1]], ids=[f"{c[0]}-{p}" for c in HEAD_CASES for p in c[1]])
def test_head_kernel_exact(ops, case, prec):
    name, _, B, H, W, C0, C1, rows, use_skip, scale = case
    assert expected_kernel(prec, C0, C1) in ("HEAD", "HEADF"), f"{name}: no longer a head-kernel case in {prec}"
    run_exact(ops, name, prec, B, H, W, C0, C1, 4, 3, B if rows == "B" else rows, use_skip, scale)


# (b) Cout = 4 calls the head kernels decline: the same exact result from the direct kernel.  name, precisions, B, H, W, C0, C1,
# bias_rows, skip, scale, stats, tile
FALLBACK_CASES = [
    ("odd_chunks_96", ("bf16",), 2, 20, 36, 96, 0, "B", True, 0.5, False, 0),          # 3 chunks (fp32: 6, a head case)
    ("odd_chunks_80", ("bf16", "fp32"), 1, 24, 8, 80, 0, 1, False, 1.0, False, 0),    # 3 / 5 chunks
    ("odd_chunks_cat40_24", ("bf16", "fp32"), 3, 16, 16, 40, 24, 1, True, 1.0, False, 0),   # 2 + 1 / 3 + 2 chunks
    ("c576_no_affine", ("bf16", "fp32"), 1, 20, 36, 576, 0, 1, True, 0.5, False, 0),  # over the 512-channel LDS limit
    ("want_stats", ("bf16", "fp32"), 2, 20, 36, 128, 0, "B", True, 1.0, True, 0),
    ("tile_bn32", ("bf16", "fp32"), 3, 16, 16, 128, 0, 1, False, 0.5, False, 32),
]


@pytest.mark.parametrize("prec,case", [(p, c) for c in FALLBACK_CASES for p in c[1]], ids=[f"{c[0]}-{p}" for c in FALLBACK_CASES for p in c[1]])
def test_head_fallback_exact(ops, case, prec):
    name, _, B, H, W, C0, C1, rows, use_skip, scale, stats, tile = case
    assert expected_kernel(prec, C0, C1, stats=stats, tile=tile) == "DIRECT", f"{name}: no longer a fallback case in {prec}"
    run_exact(ops, name, prec, B, H, W, C0, C1, 4, 3, B if rows == "B" else rows, use_skip, scale, stats=stats, tile=tile)


@pytest.mark.parametrize("prec", ["bf16", "fp32"])
def test_head_persist_flag_dispatch(ops, prec):
    """FD_TILE_PERSIST is no workgroup width: a bf16 Cout = 4 call keeps the head kernel, an fp32 one goes to the direct kernel."""
    ran = run_exact(ops, "persist_flag", prec, 2, 16, 32, 64, 0, 4, 3, 1, True, 0.5, tile="persist")
    assert ran == ("HEAD" if prec == "bf16" else "DIRECT")


# ---------------------------------------------------------------------------------------------------------
# (c) ACT = true: GroupNorm affine + SiLU folded into the operand load
# ---------------------------------------------------------------------------------------------------------
U = 2.0 ** -24


def half_ulp_bf16(v):
    """Half a bf16 ulp of |v| (0 at 0): the largest error of one round-to-nearest to bf16 of a value of that magnitude."""
    m, e = np.frexp(np.abs(v))
    return np.where(m == 0, 0.0, np.ldexp(1.0, e - 9))


# name, B, H, W, C0, C1, bias_rows, skip, scale, mean of d (d ~ +2: silu(d) != 0, so padding zeroed BEFORE the activation would add
# silu(d) * w at every image border)
ACT_CASES = [
    ("c128_d2_skip", 2, 20, 36, 128, 0, "B", True, 0.5, 2.0),
    ("c256_d0", 3, 48, 80, 256, 0, 1, False, 1.0, 0.0),
    ("cat96_32_d2", 1, 24, 8, 96, 32, "B", True, 1.0, 2.0),
    ("cat8_8_d2", 9, 1, 16, 8, 8, 0, False, 0.5, 2.0),
    ("c512_affc512_d2", 1, 20, 36, 512, 0, 1, True, 0.5, 2.0),
    ("c56_partial_d2", 3, 16, 16, 56, 0, "B", False, 1.0, 2.0),
]


@pytest.mark.parametrize("prec", ["bf16", "fp32"])
@pytest.mark.parametrize("case", ACT_CASES, ids=[c[0] for c in ACT_CASES])
def test_head_kernel_affine(ops, case, prec):
    """out = scale * (conv3x3(silu(a x + d)) + bias + skip) through the head kernels' ACT = true instantiations.  SiLU makes exactness
    impossible, so: the two relative-L2 bounds of test_conv2d, and an element-wise worst-case bound
        |got - ref| <= (K + 8) 2^-24 (sum |w| |xin| + |bias| + |skip|) scale   [+ half a bf16 ulp of the result in bf16],  K = 9 Cin.
    Derivation: f32 arithmetic, unit roundoff u = 2^-24; a sum of terms t_i computed with at most n roundings on each term's path is
    within n u sum |t_i| of the exact sum (first order).  bf16: the products of bf16 operands are exact, the accumulation chain has fewer
    than K additions, the epilogue adds bias and skip (2 more) and scales by a power of two: K + 2 <= K + 8; the one rounding of the
    store to bf16 is the half ulp.  fp32: conv_headf.hip alternates two accumulators (K/2 additions each, then one to join them), the
    product is rounded once, the epilogue adds 2, and the activated operand itself carries at most 13 u (fmaf, __expf at |a x + d| <= 5,
    1 + e, reciprocal, multiply): K/2 + 17 <= K + 8 for every K >= 18.  In bf16 the operand is rounded to bf16 first -- `ref` does the
    same -- so an activation error of 13 u can only matter for an operand within 16 u of a bf16 rounding midpoint, which may then round
    to the neighbouring bf16 value: those operands are found below, and each adds |w| * |difference of its two roundings| to the bound."""
    name, B, H, W, C0, C1, rows, use_skip, scale, dmean = case
    bias_rows = B if rows == "B" else rows
    rng = np.random.default_rng(zlib.crc32(f"act/{name}/{prec}".encode()))
    q = bf16r if prec == "bf16" else (lambda a: np.asarray(a, np.float32))
    Cin = C0 + C1
    K = 9 * Cin
    x = q(rng.uniform(-2, 2, (B, Cin, H, W))).astype(np.float64)
    w = q(rng.standard_normal((4, Cin, 3, 3)) / np.sqrt(K)).astype(np.float64)
    a = rng.uniform(0.75, 1.25, (B, Cin)).astype(np.float32)
    d = (dmean + rng.uniform(-0.5, 0.5, (B, Cin))).astype(np.float32)
    xin = O.silu(x * a[:, :, None, None].astype(np.float64) + d[:, :, None, None].astype(np.float64))
    amb = np.zeros_like(xin)
    if prec == "bf16":
        lo = bf16r(xin * (1 - 16 * U)).astype(np.float64)
        hi = bf16r(xin * (1 + 16 * U)).astype(np.float64)
        amb = np.abs(hi - lo)
        xin = bf16r(xin).astype(np.float64)    # the kernel rounds the activated operand to bf16 before the MFMA
    ref = O.conv2d(xin, w, None)
    mag = O.conv2d(np.abs(xin), np.abs(w), None)
    slack = O.conv2d(amb, np.abs(w), None)
    bias = None
    if bias_rows:
        bv = rng.standard_normal((bias_rows, 4)).astype(np.float32).astype(np.float64)
        ref = ref + bv[:, :, None, None]
        mag = mag + np.abs(bv)[:, :, None, None]
        bias = dev((bv if bias_rows > 1 else bv[0]).astype(np.float32))
    skip = None
    if use_skip:
        sk = q(rng.standard_normal((B, 4, H, W))).astype(np.float64)
        ref = ref + sk
        mag = mag + np.abs(sk)
        skip = nhwc(sk.astype(np.float32), DT[prec])
    ref, mag, slack = ref * scale, mag * scale, slack * scale
    bound = (K + 8) * U * mag + slack
    if prec == "bf16":
        bound = bound + half_ulp_bf16(np.abs(ref) + bound)
    aff = dev(np.stack([a, d], axis=-1))
    x0 = nhwc(x[:, :C0].astype(np.float32), DT[prec])
    x1 = nhwc(x[:, C0:].astype(np.float32), DT[prec]) if C1 else None
    pw = ops.pack_conv_weight(dev(w.astype(np.float32)), C0=C0, dtype=DT[prec])
    out, delta = counted(ops, lambda: ops.conv2d(x0, pw, 4, 3, x1=x1, affine=aff, bias=bias, skip=skip, scale=scale))
    kernel = expected_kernel(prec, C0, C1)
    assert kernel in ("HEAD", "HEADF"), f"{name}: no longer a head-kernel case in {prec}"
    assert_launched(delta, kernel, 1, name)
    got = from_nhwc(out).astype(np.float64)
    err = np.abs(got - ref)
    worst = float((err / bound).max())
    e2 = rel_err(got, ref)
    tol = 6e-3 if prec == "bf16" else 2e-5
    report_line(f"{'conv_head_affine[' + name + ',' + prec + ']':60s} err={e2:.3e} tol={tol:.1e} worst/bound={worst:.3f} "
                f"kernel={kernel}+{delta[kernel]} {'OK' if worst <= 1 and e2 < tol else 'FAIL'}")
    assert e2 < tol, f"{name}[{prec}]: rel err {e2:.3e} >= {tol:.1e}"
    if prec == "bf16":
        e3 = rel_err(got, bf16r(ref))
        assert e3 < 4e-4, f"{name}: rel err {e3:.3e} to the bf16-rounded numerics model"
    i = np.unravel_index(np.argmax(err / bound), err.shape)
    assert worst <= 1.0, f"{name}[{prec}]: |got - ref| = {err[i]:.3e} > bound {bound[i]:.3e} at (b, c, h, w) = {i}"


# ---------------------------------------------------------------------------------------------------------
# (d) determinism and batch independence of both head kernels
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["bf16", "fp32"])
def test_head_kernel_deterministic_and_batch_independent(ops, prec):
    """Two launches give the same bits, and image b of a B = 9 launch gives the bits of a B = 1 launch with its own affine and bias rows
    (ragged batching -- fd_enhance_ragged -- promises every file the bits of its one-file call).  Ragged tiles, two segments."""
    rng = np.random.default_rng(5 if prec == "bf16" else 6)
    B, H, W, C0, C1 = 9, 20, 36, 96, 32
    dt = DT[prec]
    x = torch.from_numpy(rng.standard_normal((B, H, W, C0 + C1)).astype(np.float32)).cuda().to(dt)
    x0, x1 = x[..., :C0].contiguous(), x[..., C0:].contiguous()
    w = dev((rng.standard_normal((4, C0 + C1, 3, 3)) / 30).astype(np.float32))
    pw = ops.pack_conv_weight(w, C0=C0, dtype=dt)
    aff = dev(np.stack([1 + 0.2 * rng.standard_normal((B, C0 + C1)), 0.3 * rng.standard_normal((B, C0 + C1))], -1).astype(np.float32))
    bias = dev(rng.standard_normal((B, 4)).astype(np.float32))
    skip = torch.from_numpy(rng.standard_normal((B, H, W, 4)).astype(np.float32)).cuda().to(dt)
    kernel = expected_kernel(prec, C0, C1)
    assert kernel in ("HEAD", "HEADF")

    def calls():
        outs = [ops.conv2d(x0, pw, 4, 3, x1=x1, affine=aff, bias=bias, skip=skip, scale=0.5) for _ in range(2)]
        ones = [ops.conv2d(x0[b:b + 1].contiguous(), pw, 4, 3, x1=x1[b:b + 1].contiguous(), affine=aff[b:b + 1].contiguous(),
                           bias=bias[b:b + 1].contiguous(), skip=skip[b:b + 1].contiguous(), scale=0.5) for b in range(B)]
        return outs, ones

    (outs, ones), delta = counted(ops, calls)
    assert_launched(delta, kernel, 2 + B, f"batch_independence[{prec}]")
    assert torch.equal(outs[0], outs[1])
    for b in range(B):
        assert torch.equal(ones[b][0], outs[0][b]), f"image {b}: the B = 1 launch differs from its slice of the B = {B} launch"
    assert torch.isfinite(outs[0].float()).all() and float(outs[0].float().abs().max()) > 0
    report_line(f"{'conv_head_batch_independent[' + prec + ']':60s} bit-identical kernel={kernel}+{delta[kernel]} OK")


# ---------------------------------------------------------------------------------------------------------
# (e) the direct kernel family on exact data: the shapes of test_hip_ops.CONV_CASES, every workgroup width, the bf16-operand modes
# ---------------------------------------------------------------------------------------------------------
MODES = {"bf16": ("bf16", False), "fp32": ("fp32", False), "mixed": ("fp32", True), "bf16x3": ("fp32", "x3")}


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("case", CONV_CASES, ids=[c[0] for c in CONV_CASES])
def test_conv2d_exact(ops, case, mode):
    """Every CONV_CASES shape without the affine (and without statistics: what test_conv2d checks with tolerances, here exactly).
    The Cout = 4 rows go where the dispatch rule sends them (the mirror decides, the counter checks)."""
    name, B, H, W, C0, C1, Cout, k, _, bias_rows, use_skip, S0, S1 = case
    prec, operands = MODES[mode]
    run_exact(ops, name, prec, B, H, W, C0, C1, Cout, k, bias_rows, use_skip, 0.5 if use_skip else 1.0, S0=S0, S1=S1, operands=operands)


# name, B, H, W, C0, C1, Cout, bias_rows, skip, S0
TILE_SHAPES = [
    ("whole_tiles_256", 2, 32, 32, 64, 32, 256, 1, False, 0),       # FD_TILE_PERSIST takes its register-epilogue kernel here (bf16)
    ("whole_tiles_128", 1, 32, 16, 128, 0, 128, 0, False, 0),       # ... and here
    ("ragged_skip_128", 3, 24, 40, 96, 0, 128, "B", True, 0),
    ("shortcut_256", 1, 16, 32, 128, 0, 256, 1, False, 64),
]


@pytest.mark.parametrize("prec", ["bf16", "fp32"])
@pytest.mark.parametrize("tile", [32, 64, 128, "64c", "32c", "duo", "persist"], ids=lambda t: f"tile_{t}")
@pytest.mark.parametrize("case", TILE_SHAPES, ids=[c[0] for c in TILE_SHAPES])
def test_conv2d_exact_tile_widths(ops, case, tile, prec):
    name, B, H, W, C0, C1, Cout, rows, use_skip, S0 = case
    run_exact(ops, f"{name}_{tile}", prec, B, H, W, C0, C1, Cout, 3, B if rows == "B" else rows, use_skip, 0.5 if use_skip else 1.0,
              S0=S0, tile=tile)


# ---------------------------------------------------------------------------------------------------------
# model level: which kernel the pyramid heads of a full-width NCSN++ forward run
# ---------------------------------------------------------------------------------------------------------
# One eager fd_ncsnpp_forward is ONE launching walk of model.hip's Fwd::run (its planning walks, forward_ws_bytes, are dry and never
# call fd_conv2d).  G10 (nf = 64, ch_mult (4, 4, 4, 2), one ResBlock per level) walks 20 ResBlocks (7 down, 2 middle, 11 up) of two
# fd_conv2d calls each (Conv_2 is folded into Conv_1), 4 pyramid heads (inputs 256 / 256 / 256 / 128 channels: even chunk counts in
# both precisions) and the input convolution, which bf16 runs on its own vector kernel (768 x 64 is whole 16 x 16 tiles, 64 couts).
MODEL_CONVS = {"bf16": 44, "fp32": 45, "bf16x3": 45}


@pytest.mark.parametrize("prec", ["bf16", "fp32", "bf16x3"])
def test_model_heads_run_the_head_kernels(ops, prec):
    import flowdec_amd
    g = np.load(os.path.join(ROOT, "tests", "golden", "g10_ncsnpp_nf64.npz"))
    m = flowdec_amd.from_preset("flowdec_75m", precision=prec)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in O.random_state_dict(seed=int(g["seed"]), nf=64).items()}, strict=False)
    m = m.cuda()
    x, y = (torch.from_numpy(np.ascontiguousarray(g[k])).cuda() for k in ("x", "y"))
    out, delta = counted(ops, lambda: m.backbone(x, y, torch.tensor([0.5], device="cuda")))
    assert torch.isfinite(torch.view_as_real(out)).all()
    moved = {k: v for k, v in delta.items() if v}
    report_line(f"{'model_conv_dispatch[nf64,' + prec + ']':60s} {moved}")
    assert sum(delta.values()) == MODEL_CONVS[prec], moved
    if prec == "bf16":
        assert delta["HEAD"] == 4 and delta["HEADF"] == 0, moved
    elif prec == "fp32":
        assert delta["HEADF"] == 4 and delta["HEAD"] == 0, moved
    else:
        assert delta["HEAD"] == 0 and delta["HEADF"] == 0 and delta["DIRECT_SPLIT"] == MODEL_CONVS[prec], moved
    del m
