"""The premises and the teeth of the exact-arithmetic Winograd tests (tests/test_hip_wino_exact.py), without a GPU.

For EVERY case of the GPU file (wino_exact_data.ALL_CASES and BATCH_CASES):
  * max |V| of the transformed input is below 2048: integers up to 2048 are exact in fp16, in packed fp16 arithmetic in any order
    (conv_wino.hip, conv_wino4.hip hold V in fp16; measured: 56 for F(2,3), 184 for F(4,3), 1176 for the 2-D form, which is f32);
  * the partial-sum bound sum_xi |A^T| sum |U| |V| + shortcut + bias + residual, which covers any partial sum in any order, is below
    2^24 quanta, so every float32 operation of the kernel is exact.  Largest: 0.126 x 2^24 for the 1-D forms (Cin = 512 with the
    activation); the 2-D form's U lives on a grid 576 times finer than its weights, its widest cases (Cin = 512, thinned to a density
    of 1/16 and 1/32) reach 0.87 x 2^24;
  * the float64 reference is exactly representable in float32.
The statistics premise: sum |y| over a 16 x 16 tile is below 2^24 output quanta in EVERY (image, tile, cout) column of every case, so
that the kernels' sum y is exact in any order (make_case balances each cout's weights, |sum g| <= 30: with the activation an output is
about 24 q x 22 x sum g).

conv_wino44f.hip: the float32 emulation of its arithmetic (wino_exact_data.emulate_f44_f32: the pack kernel's U = G g G^T with integer
numerators and one division, sequential float32 accumulation, float32 output transform) on its two largest cases has a maximum error of
0 quanta (measured: 0.0 and 0.0; required: <= 1/64 quantum, an eighth of the GPU test's cap of 1/8 quantum) -- with weights on the
72 q grid the 2-D form is exact as well, and the GPU test asserts equality.

The method has teeth: each of four planted defects of the kind a relative-L2 tolerance cannot see -- a dropped (tap, channel) of one cout, padding
zeroed before the activation, the scale-table row of the neighbouring cout, the last chunk skipped for one cout block -- makes the same
comparison the GPU test uses fail on the same data."""
import numpy as np
import pytest

import wino_exact_data as D
from oracle import flowdec_oracle as O


@pytest.mark.parametrize("kernel,case", D.ALL_CASES + list(D.BATCH_CASES.items()), ids=D.ALL_IDS + [f"{k}-{c[0]}" for k, c in D.BATCH_CASES.items()])
def test_premises(kernel, case):
    c = D.make_case(kernel, case)
    storage, _, form = D.KERNELS[kernel]
    Cout = c.Cout
    # the data class itself
    assert np.array_equal(c.x, np.round(c.x)) and np.abs(c.x).max() <= 2
    assert len(np.unique(c.q)) == 5 and all(not c.w[r].any() for r in D.zero_rows(Cout)) and np.count_nonzero(np.abs(c.w).sum(axis=(1, 2, 3)) == 0) == 2
    assert np.array_equal(c.w, 24 * c.q[:, None, None, None] * c.g) and np.abs(c.g).max() == c.gmul
    if c.act:
        assert c.z.min() >= 17 and c.z.max() <= 28 and set(np.unique(c.a)) == {1.0, 2.0} and c.d.min() >= 21 and c.d.max() <= 24
        assert len(np.unique(c.d)) >= 3 and (c.B == 1 or np.any(c.a[0] != c.a[1]) and np.any(c.d[0] != c.d[1]))   # per (b, c)
    if c.skip is not None:
        assert np.abs(c.skip).max() <= 64
    for t in (c.x, c.w, c.xs, c.ws, c.skip):                                       # storable without rounding: bf16 has 8 significant bits
        if t is not None:
            assert D.exact_in_f32(t) and (storage != "bf16" or np.array_equal(O.round_bf16(t.astype(np.float32)), t.astype(np.float32)))
    vmax, bound = D.premise(c)
    print(f"{kernel} {c.name}: max|V| = {vmax:.0f}, partial-sum bound = {bound / 2 ** 24:.3f} x 2^24")
    assert vmax < 2048                                                             # (needed where V is fp16; true of the f32 kernels' cases too)
    assert bound < 2 ** 24
    assert D.exact_in_f32(c.ref)
    # statistics: sum |y| per tile in output quanta
    ts = D.tile_sums(np.abs(c.ref), 1) / (c.q * c.scale)[None, None, :]
    print(f"{kernel} {c.name}: max tile sum |y| = {ts.max() / 2 ** 24:.3f} x 2^24 quanta")
    assert ts.max() < 2 ** 24, f"{np.count_nonzero(ts >= 2 ** 24)} tile columns reach 2^24 quanta of sum |y|"
    assert np.abs(c.g.sum(axis=(1, 2, 3))).max() <= D.G_SUM_MAX


def test_f23_form_of_f43_data():
    """premise() knows all three forms: the F(4,3) data is exact under F(2,3) too (even multiples), with a smaller bound."""
    c = D.make_case("WINO4", D.WINO4_CASES[1])
    v2, b2 = D.premise(c, "f23")
    v4, b4 = D.premise(c, "f43")
    assert v2 <= 56 and v4 <= 184 and b2 < b4 < 2 ** 24


def test_wino44f_emulation_error():
    """The float32 emulation of conv_wino44f.hip on its two largest cases (most multiply-adds per output): <= 1/64 quantum."""
    cases = sorted(D.WINO44F_CASES, key=lambda k: -(k[4] + k[5] + k[11] + k[12]) * 1000 - k[1] * k[2] * k[3])[:2]
    for case in cases:
        c = D.make_case("WINO44F", case)
        err = float(np.abs(D.emulate_f44_f32(c).astype(np.float64) - c.ref).max() / c.q.min())
        print(f"WINO44F {c.name}: emulation max err = {err:.4f} quanta")
        assert err <= 1 / 64


MUTATION_CASES = [("WINO4", "t1_c32_act_skip"), ("WINO4", "g3_c64_act_sc32")]


@pytest.mark.parametrize("kernel,name", MUTATION_CASES, ids=[n for _, n in MUTATION_CASES])
def test_emulation_is_exact_and_mutations_fail(kernel, name):
    case = next(k for k in D.CASES[kernel] if k[0] == name)
    c = D.make_case(kernel, case)
    for storage in ("bf16", "fp32"):
        store = (lambda a: O.round_bf16(a.astype(np.float32))) if storage == "bf16" else (lambda a: a)   # the one rounding of the store
        assert len(D.mismatches(store(D.emulate_f43(c)), c.ref, storage)) == 0   # the emulation of the sound kernel passes ...
        for mutation in D.MUTATIONS:                                              # ... and every planted defect fails
            idx = D.mismatches(store(D.emulate_f43(c, mutation)), c.ref, storage)
            print(f"{name} {storage} {mutation}: {len(idx)} mismatches{D.describe_mismatches(idx, c)}")
            assert len(idx) > 0, f"{mutation} passes the comparison on {name} ({storage})"
    # where the defects show: only border outputs for the padding, only the last cout block for the skipped chunk
    idx = D.mismatches(D.emulate_f43(c, "pad_before_act"), c.ref, "fp32")
    assert all(h in (0, c.H - 1) or w in (0, c.W - 1) for _, _, h, w in idx)
    idx = D.mismatches(D.emulate_f43(c, "skip_last_chunk"), c.ref, "fp32")
    assert idx[:, 1].min() >= c.Cout - 128
    # and a relative-L2 tolerance of 4e-3 does not see the dropped tap
    got = D.emulate_f43(c, "drop_tap")
    assert np.linalg.norm(got - c.ref) / np.linalg.norm(c.ref) < 4e-3
