"""Exact-arithmetic parity of the four Winograd convolution kernels: conv_wino.hip (F(2,3), bf16), conv_wino4.hip (F(4,3), bf16 storage,
fp16 operands), conv_wino4f.hip (F(4,3), f32) and conv_wino44f.hip (2-D F(4x4, 3x3), f32).

The relative-L2 tolerances of test_hip_configs.py (6e-3 / 4e-3 in bf16, 5e-6 in f32) leave room for a few dozen garbage outputs, a
dropped (tap, channel) at one image corner, a stale ring slot on the last chunk of one wave or the wrong scale-table row for one cout.
On the data of tests/wino_exact_data.py -- weights on a 24 * 2^-k grid (72 * 2^-k for the 2-D form), integer activations, an affine
under which silu(a x + d) is the integer a x + d -- every transform, product and partial sum of these kernels is exact, so
    bf16 storage:  got == bf16(ref),    f32 storage:  got == ref,    zero mismatches,
against the float64 convolution, with exactly one launch of the expected kernel.  tests/test_wino_exact_cpu.py proves the premises of
every case (max |V| < 2048, partial sums < 2^24 quanta, ref exact in f32) and that the comparison fails on four planted defects.

conv_wino44f.hip: its pack kernel forms U = G g G^T from integer numerators with one division, so the same holds (equality; the report
line also carries max err / quantum against the cap of 1/8 quantum, quantum = the smallest per-cout q of the case).

Statistics output: sum y per (image, tile, cout) equals the exact sum (sum |y| < 2^24 output quanta in every column: asserted per case
in test_wino_exact_cpu.py), sum y^2 is within 257 * 2^-24 relative (at most 256 additions of products that are each rounded once),
padded cout columns are zero.

The ACT cases rest on fd_silu(u) == u for u >= 17, which test_silu_premise asserts first.  Should it ever fail, the ACT cases FAIL
with it (they are not skipped): an element-wise-bound variant of them, as test_hip_conv_exact.test_head_kernel_affine has for the
head kernels, is deliberately not implemented -- the premise is three correctly rounded float32 operations and holds on gfx950.

The F(4,3) kernels run every case a second time with reversed_tiles=True (and without the statistics output): the same bits."""
import types

import numpy as np
import pytest
import torch

import wino_exact_data as D
from test_hip_conv_exact import DT, assert_launched, counted, dev, from_nhwc, nhwc, ops, report_line  # noqa: F401 (ops: the fixture)

pytestmark = pytest.mark.gpu

U = 2.0 ** -24


def f32(a):
    return np.asarray(a, np.float32)


# ---------------------------------------------------------------------------------------------------------
# the premise of the ACT cases: fd_silu(u) == u for u >= 17
# ---------------------------------------------------------------------------------------------------------
def silu_premise(ops):
    """gn_silu_apply (fd_silu(fmaf(x, a, d)), the expression the conv kernels fuse) in f32 on every integer u = a x + d in 17 .. 60 with
    a in {1, 2}: (the u that came out differently, how many were tried)."""
    chans = [(1.0, 17.0, 0), (2.0, 17.0, 0), (2.0, 18.0, 0), (1.0, 21.0, -4), (2.0, 21.0, -2), (2.0, 24.0, -3), (1.0, 24.0, -7), (2.0, 22.0, -2)]
    a, d, off = (np.array(v) for v in zip(*chans))
    p = np.arange(44.0)[:, None]
    x = np.clip(p + off[None, :], np.ceil((17 - d) / a), np.floor((60 - d) / a))          # [44 pixels, 8 channels], integers
    u = x * a + d
    for k in (1.0, 2.0):
        assert set(u[:, a == k].ravel()) == set(np.arange(17.0, 61.0)), "the premise test does not cover 17 .. 60"
    out = ops.gn_silu_apply(dev(f32(x.reshape(1, 1, 44, 8))), dev(f32(np.stack([a, d], -1))[None]))
    got = out.cpu().numpy().reshape(44, 8)
    return sorted(set(u[got != f32(u)].ravel())), u.size


@pytest.fixture(scope="module")
def silu_exact(ops):
    return not silu_premise(ops)[0]


def test_silu_premise(ops):
    bad, n = silu_premise(ops)
    report_line(f"{'wino_exact_premise[silu(u) == u, u = 17 .. 60]':60s} mismatches={len(bad)} of {n} tol=exact {'OK' if not bad else 'FAIL'}")
    assert not bad, f"fd_silu(u) != u in float32 for u in {bad}: the ACT cases of this file cannot be exact"


# ---------------------------------------------------------------------------------------------------------
# one case on the GPU
# ---------------------------------------------------------------------------------------------------------
def device_tensors(ops, kernel, c):
    storage, wino, _ = D.KERNELS[kernel]
    dt = DT[storage]
    t = types.SimpleNamespace(wino=wino)
    t.x0 = nhwc(f32(c.x[:, :c.C0]), dt)
    t.x1 = nhwc(f32(c.x[:, c.C0:]), dt) if c.C1 else None
    t.aff = dev(f32(np.stack([c.a, c.d], axis=-1))) if c.act else None
    t.sc0 = t.sc1 = w_sc = None
    if c.S0:
        t.sc0 = nhwc(f32(c.xs[:, :c.S0]), dt)
        t.sc1 = nhwc(f32(c.xs[:, c.S0:]), dt) if c.S1 else None
        w_sc = dev(f32(c.ws)[:, :, None, None])
    t.bias = None if c.bias is None else dev(f32(c.bias if c.bias_rows > 1 else c.bias[0]))
    t.skip = None if c.skip is None else nhwc(f32(c.skip), dt)
    t.pw = ops.pack_conv_weight(dev(f32(c.w)), C0=c.C0, dtype=dt, w_sc=w_sc, S0=c.S0 if c.S0 else None, winograd=wino)
    return t


def launch(ops, c, t, images=slice(None), **kw):
    pick = lambda v: None if v is None else v[images].contiguous()
    bias = t.bias if t.bias is None or t.bias.ndim == 1 else t.bias[images].contiguous()
    return ops.conv2d(pick(t.x0), t.pw, c.Cout, 3, x1=pick(t.x1), affine=pick(t.aff), bias=bias, skip=pick(t.skip), scale=c.scale,
                      sc0=pick(t.sc0), sc1=pick(t.sc1), winograd=t.wino, **kw)


def check_stats(stats, c, name):
    st = stats.double().cpu().numpy()                                # [B, tiles, CoutPad, 2]
    assert st.shape[:2] == (c.B, -(-c.H // 16) * -(-c.W // 16)) and st.shape[2] >= c.Cout
    assert not st[:, :, c.Cout:].any(), f"{name}: padded cout columns of the statistics are not zero"
    s1, s2 = D.tile_sums(c.ref, 1), D.tile_sums(c.ref, 2)
    d1 = st[:, :, :c.Cout, 0] != s1
    assert not d1.any(), f"{name}: sum y differs from the exact sum in {np.count_nonzero(d1)} (image, tile, cout) columns"
    d2 = np.abs(st[:, :, :c.Cout, 1] - s2)
    assert (d2 <= 257 * U * s2).all(), f"{name}: sum y^2 is off by {float((d2 / np.maximum(s2, 1e-300)).max()):.3e} relative (> 257 * 2^-24)"


@pytest.mark.parametrize("kernel,case", D.ALL_CASES, ids=D.ALL_IDS)
def test_wino_exact(ops, silu_exact, kernel, case):
    c = D.make_case(kernel, case)
    storage = D.KERNELS[kernel][0]
    name = f"{kernel},{c.name}"
    assert silu_exact or not c.act, "fd_silu(u) != u for some u >= 17 (test_silu_premise): this ACT case cannot be exact"
    t = device_tensors(ops, kernel, c)
    torch.cuda.synchronize()
    (out, stats), delta = counted(ops, lambda: launch(ops, c, t, want_stats=True))
    got = from_nhwc(out).astype(np.float64)
    idx = D.mismatches(got, c.ref, storage)
    errq = float(np.abs(got - c.ref).max() / c.q.min())             # (bf16: includes the rounding of the store)
    cap = f" err/quantum={errq:.4f} cap=0.125" if kernel == "WINO44F" else ""
    ok = len(idx) == 0 and delta.get(kernel, 0) == 1
    report_line(f"{'wino_exact[' + name + ']':60s} kernel={kernel}+{delta.get(kernel, 0)} mismatches={len(idx)} tol=exact{cap}"
                f"{D.describe_mismatches(idx, c)} {'OK' if ok else 'FAIL'}")
    if kernel == "WINO44F":
        assert errq <= 0.125, f"{name}: max |got - ref| = {errq:.4f} quanta > 1/8{D.describe_mismatches(idx, c)}"
    assert len(idx) == 0, f"{name}: {len(idx)} of {got.size} outputs differ from the exact result:{D.describe_mismatches(idx, c)}"
    assert_launched(delta, kernel, 1, name)
    check_stats(stats, c, name)
    if kernel in ("WINO4", "WINO4F"):
        out_r, delta = counted(ops, lambda: launch(ops, c, t, reversed_tiles=True))
        assert_launched(delta, kernel, 1, name + ",reversed")
        assert torch.equal(out, out_r), f"{name}: reversed_tiles=True (without statistics) gives other bits"


# ---------------------------------------------------------------------------------------------------------
# batch independence
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", list(D.BATCH_CASES))
def test_wino_batch_independent(ops, silu_exact, kernel):
    """Image b of a B = 3 launch (per-image affine and bias rows) has the bits of its own B = 1 launch -- both are the exact result."""
    assert silu_exact, "fd_silu(u) != u for some u >= 17 (test_silu_premise)"
    c = D.make_case(kernel, D.BATCH_CASES[kernel])
    storage = D.KERNELS[kernel][0]
    t = device_tensors(ops, kernel, c)

    def calls():
        return launch(ops, c, t), [launch(ops, c, t, images=slice(b, b + 1)) for b in range(c.B)]

    (whole, ones), delta = counted(ops, calls)
    assert_launched(delta, kernel, 1 + c.B, f"batch_independence[{kernel}]")
    assert len(D.mismatches(from_nhwc(whole).astype(np.float64), c.ref, storage)) == 0
    for b in range(c.B):
        assert torch.equal(ones[b][0], whole[b]), f"{kernel}: image {b} of the B = {c.B} launch differs from its B = 1 launch"
    report_line(f"{'wino_exact_batch_independent[' + kernel + ']':60s} bit-identical kernel={kernel}+{delta[kernel]} mismatches=0 tol=exact OK")
