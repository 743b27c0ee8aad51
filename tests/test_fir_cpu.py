"""CPU-only checks behind tests/test_hip_fir.py and tests/test_hip_ops_exact.py: the FIR kernel-selection rule (fd_fir_variant, host only)
against a Python mirror, the coverage of the GPU case table, the integer FIR reference against the oracle's operator, the exactness
premises, and the NumPy restatement of upfirdn2d against the oracle."""
import itertools

import numpy as np
import pytest
import torch

from oracle import flowdec_oracle as O
from test_hip_fir import CASES, MODEL_SHAPES, fir_norm, fir_scaled
from test_hip_ops_exact import UPFIRDN_DRAWS, upfirdn2d_f64, upfirdn_draw

FD_EINVAL = -1
DT = {"bf16": torch.bfloat16, "fp32": torch.float32}


@pytest.fixture(scope="module")
def ops():
    import __graft_entry__ as g
    g.build()
    from flowdec_amd import ops as _ops
    return _ops


# ---------------------------------------------------------------------------------------------------------
# the selection rule
# ---------------------------------------------------------------------------------------------------------
ENOUGH, FILL = 512, 768      # workgroups of 256 threads (fir_select in csrc/fir.hip)


def mirror(B, H, W, C, direction, prec, affine, want_raw, want_act):
    """Python mirror of fir_select: (family, rows, cols, vec, act, fast), None where the call is refused."""
    want_act = bool(affine and want_act)
    if not (want_raw or want_act) or min(B, H, W, C) <= 0 or direction not in (1, -1) or C % 4:
        return None
    if direction < 0 and (H % 2 or W % 2):
        return None
    half = prec == "bf16"
    vec = 8 if half and not (direction < 0 and affine) and C % 8 == 0 else 4
    R, Q = (H, W) if direction > 0 else (H // 2, W // 2)
    grid = lambda rows, cols: -(-(B * -(-R // rows) * -(-Q // cols) * (C // vec)) // 256)
    act = int(bool(affine))
    if direction > 0:
        if not affine:
            return ("UP", 1, 1, vec, 0, 0)
        if grid(8, 1) >= ENOUGH:
            return ("UP", 8, 1, vec, 1, int(H % 8 == 0 and want_raw and want_act))
        return ("UP", 2 if grid(2, 1) >= ENOUGH else 1, 1, vec, 1, 0)
    if not affine:
        return ("DOWN", 1, 1, vec, 0, 0)
    if want_act:
        for nr in (16, 8, 4):
            if grid(nr, 4) >= FILL:
                return ("DOWN_MARCH", nr, 4, 4, 1, int(want_raw and R % nr == 0 and Q % 4 == 0))
    if half and grid(4, 2) >= ENOUGH:
        return ("DOWN", 4, 2, 4, 1, 0)
    if half and grid(2, 1) >= ENOUGH:
        return ("DOWN", 2, 1, 4, 1, 0)
    if not half and grid(4, 1) >= ENOUGH:
        return ("DOWN", 4, 1, 4, 1, 0)
    return ("DOWN", 1, 1, 4, 1, 0)


# every variant the rule can return, per storage type (read off its branches)
def all_variants(prec):
    vecs = (8, 4) if prec == "bf16" else (4,)
    out = set()
    for v in vecs:
        out |= {("UP", 1, 1, v, 0, 0), ("UP", 8, 1, v, 1, 1), ("UP", 8, 1, v, 1, 0), ("UP", 2, 1, v, 1, 0), ("UP", 1, 1, v, 1, 0), ("DOWN", 1, 1, v, 0, 0)}
    out |= {("DOWN_MARCH", nr, 4, 4, 1, f) for nr in (16, 8, 4) for f in (0, 1)}
    out |= {("DOWN", 1, 1, 4, 1, 0)} | ({("DOWN", 4, 2, 4, 1, 0), ("DOWN", 2, 1, 4, 1, 0)} if prec == "bf16" else {("DOWN", 4, 1, 4, 1, 0)})
    return out


def selected(ops, B, H, W, C, direction, prec, affine, want_raw, want_act):
    try:
        return ops.fir_variant(B, H, W, C, direction, DT[prec], affine=affine, want_raw=want_raw, want_act=want_act)
    except RuntimeError:
        return None


def threshold_shapes():
    """(B, H, W, C, direction) just below and at every threshold of the rule, with C = 4 (one channel vector per pixel in both types when
    an affine is present or in float32): the workgroup count is then ceil(B * strips * column blocks / 256)."""
    out = []
    for need in (ENOUGH, FILL):
        below, at = (need - 1) * 256, (need - 1) * 256 + 1      # threads: the last count with need - 1 workgroups, the first with need
        for n in (below, at):
            out += [(1, 8, n, 4, 1), (1, 16, n // 8, 4, 1), (1, 16, n // 8 + 1, 4, 1)]                              # up: 8-row and 2-row strips
            out += [(1, 4 * nr, 8 * (n // 2 + e), 4, -1) for nr in (16, 8, 4) for e in (0, 1)]                                         # down: one strip, n blocks of 4 columns
            out += [(1, 8, 4 * n, 4, -1), (1, 4, 2 * n, 4, -1), (1, 8, 2 * n, 4, -1)]                       # down: 4x2, 2x1, 4x1 blocks
    return out


def test_selector_matches_mirror(ops):
    shapes = threshold_shapes()
    shapes += [(B, H, W, C, dr) for B in (1, 2, 8, 9) for H, W in ((2, 2), (1, 1), (3, 4), (24, 16), (62, 34), (96, 32), (192, 64), (256, 128),
                                                                  (384, 128), (488, 264), (768, 256), (768, 1024))
               for C in (4, 6, 8, 12, 64, 128, 256) for dr in (1, -1)]
    shapes += [(0, 8, 8, 8, 1), (1, 0, 8, 8, 1), (1, 8, 8, 8, 0), (1, 8, 8, 8, 2), (1, 8, 8, 0, -1)]
    seen = {"bf16": set(), "fp32": set()}
    n = 0
    for (B, H, W, C, dr), prec, (affine, want_raw, want_act) in itertools.product(
            shapes, ("bf16", "fp32"), ((False, True, False), (True, True, True), (True, False, True), (True, True, False), (False, False, False))):
        want = mirror(B, H, W, C, dr, prec, affine, want_raw, want_act)
        got = selected(ops, B, H, W, C, dr, prec, affine, want_raw, want_act)
        assert got == want, f"B={B} H={H} W={W} C={C} dir={dr} {prec} affine={affine} raw={want_raw} act={want_act}: selector {got}, mirror {want}"
        if got is not None:
            seen[prec].add(got)
            n += 1
    assert n > 2000
    # the sweep reaches the whole range of the rule, and nothing outside it
    for prec in seen:
        assert seen[prec] == all_variants(prec), (prec, seen[prec] ^ all_variants(prec))


def test_selector_thresholds(ops):
    """The last shape below and the first at each threshold land on different sides of it."""
    b, a = (ENOUGH - 1) * 256, (ENOUGH - 1) * 256 + 1
    assert selected(ops, 1, 8, b, 4, 1, "fp32", True, True, True) == ("UP", 2, 1, 4, 1, 0)        # 511 workgroups of 8-row strips: 2-row strips
    assert selected(ops, 1, 8, a, 4, 1, "fp32", True, True, True) == ("UP", 8, 1, 4, 1, 1)
    assert selected(ops, 1, 16, b // 8, 4, 1, "bf16", True, True, True) == ("UP", 1, 1, 4, 1, 0)   # 8 two-row strips x b / 8 columns: 511
    assert selected(ops, 1, 16, b // 8 + 1, 4, 1, "bf16", True, True, True) == ("UP", 2, 1, 4, 1, 0)
    assert selected(ops, 1, 8, 4 * b, 4, -1, "bf16", True, True, False) == ("DOWN", 2, 1, 4, 1, 0)
    assert selected(ops, 1, 8, 4 * a, 4, -1, "bf16", True, True, False) == ("DOWN", 4, 2, 4, 1, 0)
    assert selected(ops, 1, 8, 2 * b, 4, -1, "fp32", True, True, False) == ("DOWN", 1, 1, 4, 1, 0)
    assert selected(ops, 1, 8, 2 * a, 4, -1, "fp32", True, True, False) == ("DOWN", 4, 1, 4, 1, 0)
    b, a = (FILL - 1) * 256, (FILL - 1) * 256 + 1
    for nr in (16, 8, 4):
        # two strips of nr rows (one of 2 nr) x m blocks of 4 columns: 2 m threads
        below = selected(ops, 1, 4 * nr, 8 * (b // 2), 4, -1, "fp32", True, True, True)
        assert below[0] != "DOWN_MARCH" or below[1] < nr, below
        assert selected(ops, 1, 4 * nr, 8 * (b // 2 + 1), 4, -1, "fp32", True, True, True) == ("DOWN_MARCH", nr, 4, 4, 1, 1)
        assert selected(ops, 1, 4 * nr, 8 * (b // 2 + 1), 4, -1, "bf16", True, False, True) == ("DOWN_MARCH", nr, 4, 4, 1, 0)


def test_gpu_case_table_covers_every_variant(ops):
    """Every case names the variant the selector picks for it today, every variant of the rule has a case in each storage type it exists
    in, and the conditions on the edges hold: per strip / block variant a ragged last strip and a ragged last column block."""
    ids = [(c[0], c[1]) for c in CASES]
    assert len(set(ids)) == len(ids)
    hit = {"bf16": set(), "fp32": set()}
    for name, prec, direction, B, H, W, C, affine, want_raw, want_act, expected in CASES:
        assert selected(ops, B, H, W, C, direction, prec, affine, want_raw, want_act) == expected, (name, prec)
        assert mirror(B, H, W, C, direction, prec, affine, want_raw, want_act) == expected, (name, prec)
        hit[prec].add(expected)
    for prec in hit:
        assert hit[prec] == all_variants(prec), (prec, all_variants(prec) - hit[prec])

    def some(pred):
        return any(pred(*c) for c in CASES)

    for prec in ("bf16", "fp32"):
        for nr in (16, 8, 4):     # marching strips: whole (fast) and ragged in both axes
            assert some(lambda n, p, dr, B, H, W, C, af, r, a, v: p == prec and v == ("DOWN_MARCH", nr, 4, 4, 1, 1))
            assert some(lambda n, p, dr, B, H, W, C, af, r, a, v: p == prec and v[:2] == ("DOWN_MARCH", nr) and (H // 2) % nr and (W // 2) % 4 and B >= 2)
            assert some(lambda n, p, dr, B, H, W, C, af, r, a, v: p == prec and v[:2] == ("DOWN_MARCH", 4) and not r)
        blocks = ((4, 2), (2, 1)) if prec == "bf16" else ((4, 1),)
        for by, bx in blocks:
            assert some(lambda n, p, dr, B, H, W, C, af, r, a, v: p == prec and v[:3] == ("DOWN", by, bx) and (H // 2) % by == 0 and (W // 2) % bx == 0)
            assert some(lambda n, p, dr, B, H, W, C, af, r, a, v: p == prec and v[:3] == ("DOWN", by, bx) and (H // 2) % by and (bx == 1 or (W // 2) % bx))
        for rows in (8, 2):
            assert some(lambda n, p, dr, B, H, W, C, af, r, a, v: p == prec and v[:2] == ("UP", rows) and H % rows == 0)
            assert some(lambda n, p, dr, B, H, W, C, af, r, a, v: p == prec and v[:2] == ("UP", rows) and H % rows and W % 2)
        # the degenerate images on the small kernels, a missing raw output, and out_act = NULL with an affine present
        assert some(lambda n, p, dr, B, H, W, C, af, r, a, v: p == prec and dr < 0 and H == 2 and W == 2 and af)
        assert some(lambda n, p, dr, B, H, W, C, af, r, a, v: p == prec and dr > 0 and H == 1 and af)
        assert some(lambda n, p, dr, B, H, W, C, af, r, a, v: p == prec and dr > 0 and W == 1 and af)
        assert some(lambda n, p, dr, B, H, W, C, af, r, a, v: p == prec and af and not r)
        assert some(lambda n, p, dr, B, H, W, C, af, r, a, v: p == prec and af and not a and dr > 0)
        assert some(lambda n, p, dr, B, H, W, C, af, r, a, v: p == prec and af and not a and dr < 0)
    assert some(lambda n, p, dr, B, H, W, C, af, r, a, v: dr < 0 and H == 2 and W > 2) and some(lambda n, p, dr, B, H, W, C, af, r, a, v: dr < 0 and W == 2 and H > 2)


def test_model_rows_come_from_the_network_walk():
    """MODEL_SHAPES is what one evaluation of FlowDec-75m launches: walk the module list as model.hip's Fwd::run does."""
    specs = O.build_module_specs(nf=64, ch_mult=(4, 4, 4, 2), num_res_blocks=1)
    H, W = 768, 256
    calls, pyr = [], None
    i = 4
    for lvl in range(4):                                   # down path
        assert specs[i]["kind"] == "rb" and not specs[i]["down"]
        i += 1
        if lvl != 3:
            assert specs[i]["down"] and specs[i + 1]["kind"] == "combine"
            calls.append((-1, H, W, specs[i]["cin"], True))
            calls.append((-1, H, W, 8, False))             # the input pyramid, 4 channels stored as 8
            H, W = H // 2, W // 2
            i += 2
    i += 2                                                 # the two middle blocks
    for lvl in reversed(range(4)):                         # up path
        i += 2
        assert specs[i]["kind"] == "gn" and specs[i + 1]["kind"] == "conv3"
        if pyr is not None:
            calls.append((1, pyr[0], pyr[1], 4, False))    # the output pyramid joins the head's convolution
        pyr = (H, W)
        i += 2
        if lvl != 0:
            assert specs[i]["up"]
            calls.append((1, H, W, specs[i]["cin"], True))
            H, W = 2 * H, 2 * W
            i += 1
    assert i == len(specs)
    assert sorted(calls) == sorted(m[1:] for m in MODEL_SHAPES)
    for prec in ("bf16", "fp32"):
        for B in (1, 8):
            rows = {c[2:8] for c in CASES if c[0].startswith("model_") and c[1] == prec and c[3] == B}
            assert rows == {(dr, B, h, w, ch, af) for _, dr, h, w, ch, af in MODEL_SHAPES}


# ---------------------------------------------------------------------------------------------------------
# the references
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2, 3, 8, 6), (1, 4, 2, 2), (2, 1, 2, 10), (1, 2, 12, 2), (3, 5, 14, 18)])
def test_int_reference_down_is_the_operator(shape):
    """int32 polyphase reference / 64 == O.downsample_2d (float64 upfirdn2d: pad, correlate with the flipped kernel, decimate) bit for bit."""
    rng = np.random.default_rng(sum(shape))
    x = rng.integers(-2, 3, shape)                                    # NCHW
    ref = O.downsample_2d(x.astype(np.float64))
    got = fir_scaled(np.transpose(x, (0, 2, 3, 1)).astype(np.int32), -1, (1, 2))
    assert got.dtype == np.int32
    assert np.array_equal(np.transpose(got, (0, 3, 1, 2)) / 64.0, ref)
    assert np.array_equal(O.fir_down2_polyphase(x.astype(np.float64)), ref)
    assert np.array_equal(fir_scaled(np.transpose(x, (0, 2, 3, 1))[0].astype(np.int32), -1, (0, 1)), got[0])      # the per-clip form


@pytest.mark.parametrize("shape", [(2, 3, 8, 6), (1, 4, 1, 1), (2, 1, 1, 7), (1, 2, 6, 1), (3, 5, 7, 9), (1, 1, 2, 3)])
def test_int_reference_up_is_the_operator(shape):
    rng = np.random.default_rng(sum(shape))
    x = rng.integers(-2, 3, shape)
    ref = O.upsample_2d(x.astype(np.float64))
    got = fir_scaled(np.transpose(x, (0, 2, 3, 1)).astype(np.int32), 1, (1, 2))
    assert got.dtype == np.int32
    assert np.array_equal(np.transpose(got, (0, 3, 1, 2)) / 16.0, ref)
    assert np.array_equal(O.fir_up2_polyphase(x.astype(np.float64)), ref)
    assert np.array_equal(fir_scaled(np.transpose(x, (0, 2, 3, 1))[0].astype(np.int32), 1, (0, 1)), got[0])


def test_float_reference_is_the_operator():
    """The float64 form used for the activated output: within float64 rounding of the oracle's operator on random data."""
    rng = np.random.default_rng(4)
    x = rng.standard_normal((2, 3, 10, 6))
    for direction, f in ((-1, O.downsample_2d), (1, O.upsample_2d)):
        got = np.transpose(fir_scaled(np.transpose(x, (0, 2, 3, 1)), direction, (1, 2)), (0, 3, 1, 2)) / fir_norm(direction)
        assert np.abs(got - f(x)).max() <= 1e-15


def significant_bits(v):
    """Bits between the leading and the trailing one of |v| (0 for 0)."""
    v = np.abs(np.asarray(v, np.int64))
    out = np.zeros(v.shape, np.int64)
    nz = v != 0
    low = v[nz] & -v[nz]
    out[nz] = np.floor(np.log2(v[nz])).astype(np.int64) - np.floor(np.log2(low)).astype(np.int64) + 1
    return out


def test_exactness_premises():
    """|x| <= 2: 64 x down and 16 x up are integers of at most 8 significant bits (bf16 holds 8), the worst case being the constant image;
    |x| <= 3 over a 2048-pixel tile: sums below 2^13 and sums of squares below 2^15 (float32 holds 24 bits in any order)."""
    rng = np.random.default_rng(0)
    x = rng.integers(-2, 3, (4, 40, 36, 8)).astype(np.int32)
    x[0] = 2
    x[1] = -2
    for direction in (-1, 1):
        r = fir_scaled(x, direction, (1, 2))
        assert np.abs(r).max() == 2 * fir_norm(direction)
        assert significant_bits(r).max() <= 8
        f = (r / fir_norm(direction)).astype(np.float32)
        assert np.array_equal(O.round_bf16(f), f)
    assert 2048 * 3 < 2 ** 13 and 2048 * 9 < 2 ** 15


# ---------------------------------------------------------------------------------------------------------
# the NumPy restatement of upfirdn2d (tests/test_hip_ops_exact.py) against the oracle's, where the oracle's form applies
# ---------------------------------------------------------------------------------------------------------
def test_upfirdn_restatement_matches_oracle():
    """O.upfirdn2d (pinned to the reference by the golden G4) takes one up / down factor and one pad pair for both axes; the restatement
    takes them per axis.  On such symmetric calls -- negative pads included -- the two agree exactly (integer data, dyadic kernels)."""
    rng = np.random.default_rng(1)
    n = 0
    for up, down, p0, p1 in itertools.product((1, 2, 3), (1, 2, 3), (-2, 0, 1, 3), (-1, 0, 2)):
        kh, kw = int(rng.integers(1, 5)), int(rng.integers(1, 6))
        k = rng.integers(-4, 5, (kh, kw)) / 4.0
        x = rng.integers(-3, 4, (2, 3, 7, 6)).astype(np.float64)           # NCHW for the oracle
        if 7 * up + p0 + p1 < kh or 6 * up + p0 + p1 < kw:
            continue
        ref = O.upfirdn2d(x, k, up=up, down=down, pad=(p0, p1))
        got = upfirdn2d_f64(x.reshape(6, 7, 6, 1), k, up, up, down, down, p0, p1, p0, p1)
        assert np.array_equal(got.reshape(2, 3, got.shape[1], got.shape[2]), ref), (up, down, p0, p1, kh, kw)
        n += 1
    assert n > 60


def test_upfirdn_draws_are_exact_and_varied():
    """The GPU sweep's draws: every result is exactly representable in bf16 as well (the premise of comparing for equality), and the draws
    cover negative pads, every factor and non-square kernels."""
    ups, downs, pads, ks = set(), set(), set(), set()
    for i in range(UPFIRDN_DRAWS):
        x, k, args = upfirdn_draw(i)
        ref = upfirdn2d_f64(x, k, *args)
        assert ref.size > 0
        f = ref.astype(np.float32)
        assert np.array_equal(f.astype(np.float64), ref) and np.array_equal(O.round_bf16(f), f)
        ups |= {args[0], args[1]}
        downs |= {args[2], args[3]}
        pads |= set(args[4:])
        ks.add(k.shape)
    assert ups == {1, 2, 3} and downs == {1, 2, 3} and min(pads) == -2 and max(pads) == 3
    assert {(1, 1), (4, 5), (4, 1), (1, 5)} <= ks and len(ks) > 8
