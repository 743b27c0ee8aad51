"""Every kernel variant of the FIR [1,3,3,1] x2 resampling (csrc/fir.hip: fir_up_kernel, fir_down_kernel, fir_down_march_kernel)
against an independent reference, on whole images -- borders, ragged last strips and column blocks included.

Raw output, EXACT.  The taps are 1/8, 3/8 per axis (down) and 1/4, 3/4 (up).  On integer input with |x| <= 2 every product and every
partial sum of every fma order is a multiple of 1/64 (down) or 1/16 (up) bounded by max |x|: at most 8 significant bits, exact in
float32 and exactly representable in bf16.  The reference is the polyphase FIR in int32 (fir_scaled below; tests/test_fir_cpu.py
ties it bit for bit to the oracle's upsample_2d / downsample_2d, i.e. to the zero-insert / pad / correlate / decimate operator itself).
A misplaced tap, a wrong zero-padding factor, a lost row of a strip or a wrong store guard changes some output by at least 1/64.

Activated output, ELEMENT-WISE BOUND (act_reference).  The same launch also resamples s = silu(a x + d); the reference is the float64 FIR
of the float64 silu.  With u = 2^-24 (float32 unit roundoff; "1 ulp" of a hardware instruction = 2u) and t = a x + d, sig = sigmoid(t),
the kernel computes, per operand,
    t^  = fmaf(x, a, d)                    one rounding: relative error u in t, which silu turns into |1 + t (1 - sig)| u   (the relative
                                           condition number of silu at t)
    e   = __expf(-t^) = exp2(log2e * -t^)  the float constant log2e (relative error <= u) and the product's rounding (u) shift the exponent
                                           by at most 2u |t| log2e, i.e. e by the factor 2 |t| u; v_exp_f32 adds 1 ulp: (2 |t| + 2) u
    q   = 1 + e                            the error of e enters with weight e / (1 + e) = 1 - sig; the addition rounds: + u
    r   = rcp(q)                           v_rcp_f32: 1 ulp = 2u
    s^  = t^ * r                           u
so |s^ - s| <= E(t) u |s| with  E(t) = |1 + t (1 - sig)| + (1 - sig) (2 |t| + 2) + 4  (first order; 13.5 at t = -3, 5.1 at t = +5).  The
zero-padding factor (1.0 or 0.0) is exact.  Each activated operand then reaches an output through at most 8 fused multiply-adds (4
horizontal + 4 vertical taps down; 2 + 2 up, the products with 1/4 being exact) with positive weights W_i summing to 1, each fma rounding
a partial sum no larger than sum W_i |s_i|:
    |got - ref| <= u * sum_i W_i |s_i| (E(t_i) + 8)          [+ half a bf16 ulp of the result for the store in bf16].
Nothing in this bound is fitted to what the kernels return; worst/bound per case goes to the parity report.  The suite's relative-L2
bounds (4e-3 bf16, 2e-6 fp32) are kept as well.

Every case first asserts which variant fd_fir_variant reports for it (the selector the launch itself goes through), so a case that drifts
to another kernel fails instead of silently testing something else; tests/test_fir_cpu.py checks that every variant the selector can
return has a case here."""
import os
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest
import torch

from oracle import flowdec_oracle as O
from test_hip_ops import REPORT

pytestmark = pytest.mark.gpu

DT = {"bf16": torch.bfloat16, "fp32": torch.float32}
U = 2.0 ** -24


def report_line(line):
    os.makedirs(os.path.dirname(REPORT), exist_ok=True)
    with open(REPORT, "a") as f:
        f.write(line + "\n")


@pytest.fixture(scope="module")
def ops():
    from flowdec_amd import ops as _ops
    return _ops


# ---------------------------------------------------------------------------------------------------------
# references (NumPy only; NHWC or HWC arrays, the two image axes given explicitly)
# ---------------------------------------------------------------------------------------------------------
def _down_axis(x, axis):
    """out[n] = x[2n-1] + 3 x[2n] + 3 x[2n+1] + x[2n+2] along `axis` (even length), zeros outside: 8 x the down-sampling FIR."""
    v = np.moveaxis(x, axis, 0)
    ev, od = v[0::2], v[1::2]
    out = 3 * (ev + od)
    out[1:] += od[:-1]
    out[:-1] += ev[1:]
    return np.moveaxis(out, 0, axis)


def _up_axis(x, axis):
    """out[2i] = x[i-1] + 3 x[i], out[2i+1] = 3 x[i] + x[i+1] along `axis`, zeros outside: 4 x the up-sampling FIR."""
    v = np.moveaxis(x, axis, 0)
    out = np.empty((2 * v.shape[0],) + v.shape[1:], v.dtype)
    out[0::2] = 3 * v
    out[1::2] = out[0::2]
    out[2::2] += v[:-1]
    out[1:-1:2] += v[1:]
    return np.moveaxis(out, 0, axis)


def fir_scaled(x, direction, axes):
    """The unnormalised resampling of x over the two image axes: 64 x downsample_2d (direction -1) or 16 x upsample_2d (+1).  Integer in,
    integer out (int32 for the exact reference); float64 in, float64 out."""
    f = _up_axis if direction > 0 else _down_axis
    return f(f(x, axes[0]), axes[1])


def fir_norm(direction):
    return 16 if direction > 0 else 64


def half_ulp_bf16(v):
    """Half a bf16 ulp of |v| (0 at 0): the largest error of one round-to-nearest to bf16 of a value of that magnitude."""
    m, e = np.frexp(np.abs(v))
    return np.where(m == 0, 0.0, np.ldexp(1.0, e - 9))


def act_operand(x, a, d):
    """float64 s = silu(a x + d) and the per-operand error budget E(t) + 8 in units of u (module docstring)."""
    t = x.astype(np.float64) * a.astype(np.float64) + d.astype(np.float64)
    one_minus_sig = 1.0 / (1.0 + np.exp(t))
    s = t * (1.0 - one_minus_sig)
    budget = np.abs(1.0 + t * one_minus_sig) + one_minus_sig * (2.0 * np.abs(t) + 2.0) + 4.0 + 8.0
    return s, budget


def act_reference(x, a, d, direction, bf16):
    """One clip x [H][W][C] (any real dtype), a / d [C] float32 -> (float64 reference of the activated output, element-wise bound)."""
    s, budget = act_operand(x, a, d)
    n = fir_norm(direction)
    ref = fir_scaled(s, direction, (0, 1)) / n
    bound = fir_scaled(np.abs(s) * budget, direction, (0, 1)) * (U / n)
    if bf16:
        bound = bound + half_ulp_bf16(np.abs(ref) + bound)
    return ref, bound


# ---------------------------------------------------------------------------------------------------------
# the case table
# ---------------------------------------------------------------------------------------------------------
# Every FIR launch of one network evaluation of FlowDec-75m (nf 64, ch_mult (4, 4, 4, 2), one ResBlock per level; 768 bins x T_pad = 256
# frames), from the walk of model.hip's Fwd::run (all_modules indices as in oracle.build_module_specs; tests/test_fir_cpu.py repeats the
# walk).  (origin, direction, H, W, C, affine): the ResBlocks resample x and silu(GroupNorm_0(x)) in one launch (Fwd::resblock), the
# pyramids have no affine and one output.
MODEL_SHAPES = [
    ("rb_down_m5", -1, 768, 256, 256, True),     # all_modules.5: down ResBlock leaving level 0
    ("rb_down_m8", -1, 384, 128, 256, True),     # all_modules.8: down ResBlock leaving level 1
    ("rb_down_m11", -1, 192, 64, 256, True),     # all_modules.11: down ResBlock leaving level 2
    ("pyr_in_l0", -1, 768, 256, 8, False),       # input pyramid (4 channels padded to 8) beside all_modules.6 (Combine)
    ("pyr_in_l1", -1, 384, 128, 8, False),       # ... beside all_modules.9
    ("pyr_in_l2", -1, 192, 64, 8, False),        # ... beside all_modules.12
    ("rb_up_m20", 1, 96, 32, 128, True),         # all_modules.20: up ResBlock leaving level 3
    ("rb_up_m25", 1, 192, 64, 256, True),        # all_modules.25: up ResBlock leaving level 2
    ("rb_up_m30", 1, 384, 128, 256, True),       # all_modules.30: up ResBlock leaving level 1
    ("pyr_out_l2", 1, 96, 32, 4, False),         # output pyramid before the head all_modules.24
    ("pyr_out_l1", 1, 192, 64, 4, False),        # ... before all_modules.29
    ("pyr_out_l0", 1, 384, 128, 4, False),       # ... before all_modules.34
]

# expected variant of every model row: (B, precision) -> {origin: (family, rows, cols, vec, act, fast)}
_M = "DOWN_MARCH"
MODEL_VARIANTS = {
    (1, "bf16"): {"rb_down_m5": (_M, 4, 4, 4, 1, 1), "rb_down_m8": ("DOWN", 2, 1, 4, 1, 0), "rb_down_m11": ("DOWN", 1, 1, 4, 1, 0),
                  "pyr_in_l0": ("DOWN", 1, 1, 8, 0, 0), "pyr_in_l1": ("DOWN", 1, 1, 8, 0, 0), "pyr_in_l2": ("DOWN", 1, 1, 8, 0, 0),
                  "rb_up_m20": ("UP", 1, 1, 8, 1, 0), "rb_up_m25": ("UP", 2, 1, 8, 1, 0), "rb_up_m30": ("UP", 8, 1, 8, 1, 1),
                  "pyr_out_l2": ("UP", 1, 1, 4, 0, 0), "pyr_out_l1": ("UP", 1, 1, 4, 0, 0), "pyr_out_l0": ("UP", 1, 1, 4, 0, 0)},
    (8, "bf16"): {"rb_down_m5": (_M, 16, 4, 4, 1, 1), "rb_down_m8": (_M, 8, 4, 4, 1, 1), "rb_down_m11": ("DOWN", 4, 2, 4, 1, 0),
                  "pyr_in_l0": ("DOWN", 1, 1, 8, 0, 0), "pyr_in_l1": ("DOWN", 1, 1, 8, 0, 0), "pyr_in_l2": ("DOWN", 1, 1, 8, 0, 0),
                  "rb_up_m20": ("UP", 2, 1, 8, 1, 0), "rb_up_m25": ("UP", 8, 1, 8, 1, 1), "rb_up_m30": ("UP", 8, 1, 8, 1, 1),
                  "pyr_out_l2": ("UP", 1, 1, 4, 0, 0), "pyr_out_l1": ("UP", 1, 1, 4, 0, 0), "pyr_out_l0": ("UP", 1, 1, 4, 0, 0)},
    (1, "fp32"): {"rb_down_m5": (_M, 4, 4, 4, 1, 1), "rb_down_m8": ("DOWN", 4, 1, 4, 1, 0), "rb_down_m11": ("DOWN", 1, 1, 4, 1, 0),
                  "pyr_in_l0": ("DOWN", 1, 1, 4, 0, 0), "pyr_in_l1": ("DOWN", 1, 1, 4, 0, 0), "pyr_in_l2": ("DOWN", 1, 1, 4, 0, 0),
                  "rb_up_m20": ("UP", 1, 1, 4, 1, 0), "rb_up_m25": ("UP", 2, 1, 4, 1, 0), "rb_up_m30": ("UP", 8, 1, 4, 1, 1),
                  "pyr_out_l2": ("UP", 1, 1, 4, 0, 0), "pyr_out_l1": ("UP", 1, 1, 4, 0, 0), "pyr_out_l0": ("UP", 1, 1, 4, 0, 0)},
    (8, "fp32"): {"rb_down_m5": (_M, 16, 4, 4, 1, 1), "rb_down_m8": (_M, 8, 4, 4, 1, 1), "rb_down_m11": ("DOWN", 4, 1, 4, 1, 0),
                  "pyr_in_l0": ("DOWN", 1, 1, 4, 0, 0), "pyr_in_l1": ("DOWN", 1, 1, 4, 0, 0), "pyr_in_l2": ("DOWN", 1, 1, 4, 0, 0),
                  "rb_up_m20": ("UP", 2, 1, 4, 1, 0), "rb_up_m25": ("UP", 8, 1, 4, 1, 1), "rb_up_m30": ("UP", 8, 1, 4, 1, 1),
                  "pyr_out_l2": ("UP", 1, 1, 4, 0, 0), "pyr_out_l1": ("UP", 1, 1, 4, 0, 0), "pyr_out_l0": ("UP", 1, 1, 4, 0, 0)},
}

# (name, precision, direction, B, H, W, C, affine, want_raw, want_act, expected variant)
CASES = [(f"model_{origin}_b{B}", prec, direction, B, H, W, C, affine, True, affine, MODEL_VARIANTS[(B, prec)][origin])
         for prec in ("bf16", "fp32") for B in (1, 8) for origin, direction, H, W, C, affine in MODEL_SHAPES]

# Edge rows: the smallest shapes that still reach their variant.  The selector counts workgroups of 256 threads, one thread per (clip, strip
# of `rows`, block of `cols`, channel vector): the up kernels take 8 rows from 512 workgroups (else 2 rows from 512, else 1), the marching
# down kernel the tallest of 16 / 8 / 4-row strips with 768 workgroups, the down block kernels 4x2 then 2x1 (bf16) or 4x1 (fp32) from 512.
CASES += [
    # ---- up, bf16, 8-channel vectors -------------------------------------------------------------------------------------------
    ("up8_whole", "bf16", 1, 2, 64, 256, 256, True, True, True, ("UP", 8, 1, 8, 1, 1)),
    ("up8_ragged_h60_w257", "bf16", 1, 2, 60, 257, 256, True, True, True, ("UP", 8, 1, 8, 1, 0)),       # H % 8 = 4, odd W
    ("up8_no_raw", "bf16", 1, 2, 64, 256, 256, True, False, True, ("UP", 8, 1, 8, 1, 0)),
    ("up8_no_act", "bf16", 1, 2, 64, 256, 256, True, True, False, ("UP", 8, 1, 8, 1, 0)),               # affine present, out_act NULL
    ("up2_whole", "bf16", 1, 1, 32, 256, 256, True, True, True, ("UP", 2, 1, 8, 1, 0)),
    ("up2_ragged_h31_w257", "bf16", 1, 1, 31, 257, 256, True, True, True, ("UP", 2, 1, 8, 1, 0)),       # odd H: a one-row last strip
    ("up1_small", "bf16", 1, 3, 5, 3, 16, True, True, True, ("UP", 1, 1, 8, 1, 0)),
    ("up1_h1", "bf16", 1, 2, 1, 7, 8, True, True, True, ("UP", 1, 1, 8, 1, 0)),
    ("up1_w1", "bf16", 1, 2, 6, 1, 8, True, True, True, ("UP", 1, 1, 8, 1, 0)),
    ("up1_1x1", "bf16", 1, 2, 1, 1, 8, True, True, True, ("UP", 1, 1, 8, 1, 0)),
    ("up_plain_c8", "bf16", 1, 2, 5, 3, 8, False, True, False, ("UP", 1, 1, 8, 0, 0)),
    ("up_plain_1x1", "bf16", 1, 2, 1, 1, 8, False, True, False, ("UP", 1, 1, 8, 0, 0)),
    # ---- up, bf16, 4-channel vectors (C % 8 != 0) ---------------------------------------------------------------------------------
    ("up8_c12_whole", "bf16", 1, 4, 128, 684, 12, True, True, True, ("UP", 8, 1, 4, 1, 1)),
    ("up8_c12_ragged_h124", "bf16", 1, 4, 124, 684, 12, True, True, True, ("UP", 8, 1, 4, 1, 0)),
    ("up2_c12", "bf16", 1, 1, 127, 685, 12, True, True, True, ("UP", 2, 1, 4, 1, 0)),
    ("up1_c12", "bf16", 1, 2, 3, 5, 12, True, True, True, ("UP", 1, 1, 4, 1, 0)),
    ("up1_c4_1x1", "bf16", 1, 2, 1, 1, 4, True, True, True, ("UP", 1, 1, 4, 1, 0)),
    ("up_plain_c4_w1", "bf16", 1, 2, 3, 1, 4, False, True, False, ("UP", 1, 1, 4, 0, 0)),
    # ---- up, fp32 ------------------------------------------------------------------------------------------------------------------
    ("up8_whole", "fp32", 1, 2, 64, 256, 128, True, True, True, ("UP", 8, 1, 4, 1, 1)),
    ("up8_ragged_h60_w257", "fp32", 1, 2, 60, 257, 128, True, True, True, ("UP", 8, 1, 4, 1, 0)),
    ("up8_no_raw", "fp32", 1, 2, 64, 256, 128, True, False, True, ("UP", 8, 1, 4, 1, 0)),
    ("up8_no_act", "fp32", 1, 2, 64, 256, 128, True, True, False, ("UP", 8, 1, 4, 1, 0)),
    ("up2_ragged_h31_w257", "fp32", 1, 1, 31, 257, 128, True, True, True, ("UP", 2, 1, 4, 1, 0)),
    ("up1_small", "fp32", 1, 3, 5, 3, 12, True, True, True, ("UP", 1, 1, 4, 1, 0)),
    ("up1_h1", "fp32", 1, 2, 1, 7, 4, True, True, True, ("UP", 1, 1, 4, 1, 0)),
    ("up1_w1", "fp32", 1, 2, 6, 1, 4, True, True, True, ("UP", 1, 1, 4, 1, 0)),
    ("up_plain_1x1", "fp32", 1, 2, 1, 1, 8, False, True, False, ("UP", 1, 1, 4, 0, 0)),
    # ---- down, marching strips (4-channel vectors in both types) ---------------------------------------------------------------------
    # whole strips with both outputs (the unconditional-store form) are the model rows rb_down_m5 (16 rows at B = 8, 4 rows at B = 1) and
    # rb_down_m8 (8 rows at B = 8); here the guarded form: ragged last strip and last column block, and out_raw = NULL on whole strips
    ("march16_ragged", "bf16", -1, 8, 368, 260, 256, True, True, True, (_M, 16, 4, 4, 1, 0)),            # 184 rows = 11 x 16 + 8, 130 columns = 32 x 4 + 2
    ("march16_ragged", "fp32", -1, 8, 368, 260, 256, True, True, True, (_M, 16, 4, 4, 1, 0)),
    ("march8_ragged", "bf16", -1, 8, 376, 132, 256, True, True, True, (_M, 8, 4, 4, 1, 0)),              # 188 rows = 23 x 8 + 4, 66 columns = 16 x 4 + 2
    ("march8_ragged", "fp32", -1, 8, 376, 132, 256, True, True, True, (_M, 8, 4, 4, 1, 0)),
    ("march4_ragged", "bf16", -1, 2, 380, 260, 256, True, True, True, (_M, 4, 4, 4, 1, 0)),              # 190 rows = 47 x 4 + 2, 130 columns
    ("march4_ragged", "fp32", -1, 2, 380, 260, 256, True, True, True, (_M, 4, 4, 4, 1, 0)),
    ("march4_ragged_1row_1col", "bf16", -1, 2, 386, 258, 256, True, True, True, (_M, 4, 4, 4, 1, 0)),    # 193 rows = 48 x 4 + 1, 129 columns = 32 x 4 + 1
    ("march4_no_raw", "bf16", -1, 2, 384, 256, 256, True, False, True, (_M, 4, 4, 4, 1, 0)),
    ("march4_no_raw", "fp32", -1, 2, 384, 256, 256, True, False, True, (_M, 4, 4, 4, 1, 0)),
    ("march4_whole_b2", "bf16", -1, 2, 384, 256, 256, True, True, True, (_M, 4, 4, 4, 1, 1)),
    ("march4_whole_b2", "fp32", -1, 2, 384, 256, 256, True, True, True, (_M, 4, 4, 4, 1, 1)),
    # ---- down, block kernels -------------------------------------------------------------------------------------------------------
    ("down4x2_ragged", "bf16", -1, 6, 188, 66, 256, True, True, True, ("DOWN", 4, 2, 4, 1, 0)),         # 94 rows = 23 x 4 + 2, 33 columns = 16 x 2 + 1
    ("down4x2_no_act", "bf16", -1, 2, 384, 256, 256, True, True, False, ("DOWN", 4, 2, 4, 1, 0)),       # out_act NULL keeps the strips out
    ("down4x2_no_raw", "bf16", -1, 6, 188, 66, 256, True, False, True, ("DOWN", 4, 2, 4, 1, 0)),
    ("down2x1_ragged", "bf16", -1, 2, 190, 66, 256, True, True, True, ("DOWN", 2, 1, 4, 1, 0)),         # 95 rows = 47 x 2 + 1
    ("down4x1_ragged", "fp32", -1, 3, 188, 66, 256, True, True, True, ("DOWN", 4, 1, 4, 1, 0)),         # 94 rows = 23 x 4 + 2
    ("down4x1_no_act", "fp32", -1, 2, 384, 256, 256, True, True, False, ("DOWN", 4, 1, 4, 1, 0)),
    ("down1_small", "bf16", -1, 3, 10, 6, 16, True, True, True, ("DOWN", 1, 1, 4, 1, 0)),
    ("down1_h2", "bf16", -1, 2, 2, 14, 8, True, True, True, ("DOWN", 1, 1, 4, 1, 0)),
    ("down1_w2", "bf16", -1, 2, 12, 2, 12, True, True, True, ("DOWN", 1, 1, 4, 1, 0)),
    ("down1_2x2", "bf16", -1, 2, 2, 2, 4, True, True, True, ("DOWN", 1, 1, 4, 1, 0)),
    ("down1_small", "fp32", -1, 3, 10, 6, 16, True, True, True, ("DOWN", 1, 1, 4, 1, 0)),
    ("down1_2x2", "fp32", -1, 2, 2, 2, 4, True, True, True, ("DOWN", 1, 1, 4, 1, 0)),
    ("down1_no_raw", "fp32", -1, 2, 2, 14, 8, True, False, True, ("DOWN", 1, 1, 4, 1, 0)),
    ("down_plain_c8_2x2", "bf16", -1, 2, 2, 2, 8, False, True, False, ("DOWN", 1, 1, 8, 0, 0)),
    ("down_plain_c12", "bf16", -1, 2, 10, 6, 12, False, True, False, ("DOWN", 1, 1, 4, 0, 0)),
    ("down_plain_c4_h2", "bf16", -1, 2, 2, 6, 4, False, True, False, ("DOWN", 1, 1, 4, 0, 0)),
    ("down_plain_w2", "fp32", -1, 2, 10, 2, 8, False, True, False, ("DOWN", 1, 1, 4, 0, 0)),
]


def case_id(c):
    return f"{c[0]}-{c[1]}"


def variant_name(v):
    family, rows, cols, vec, act, fast = v
    return f"{family}_{rows}x{cols}_v{vec}{'_act' if act else ''}{'_fast' if fast else ''}"


def _per_clip(fn, B):
    """fn(b) for every clip, a few at a time (NumPy releases the interpreter lock inside its loops)."""
    with ThreadPoolExecutor(max_workers=min(8, B)) as ex:
        return list(ex.map(fn, range(B)))


@pytest.mark.parametrize("case", CASES, ids=[case_id(c) for c in CASES])
def test_fir_variant_exact_and_bounded(ops, case):
    """One launch per case on integer x in [-2, 2] with a random per-clip affine (a in [0.75, 1.25], d around 0 or around +2 per channel,
    so silu(d) != 0 and padding applied before instead of after the activation shows at every border; |a x + d| <= 5 as in the ACT_CASES
    of test_hip_conv_exact.py): the raw output equals the int32 reference bit for bit on ALL outputs, the activated output of the same
    launch is within the derived element-wise bound (module docstring) of the float64 reference on all outputs of every clip."""
    name, prec, direction, B, H, W, C, affine, want_raw, want_act, expected = case
    got_variant = ops.fir_variant(B, H, W, C, direction, DT[prec], affine=affine, want_raw=want_raw, want_act=want_act)
    assert got_variant == expected, f"{name}[{prec}]: the selector now picks {got_variant}, this case was written for {expected}"
    rng = np.random.default_rng(zlib.crc32(f"fir/{name}/{prec}".encode()))
    x = rng.integers(-2, 3, (B, H, W, C), dtype=np.int8)
    a = d = aff = None
    if affine:
        a = rng.uniform(0.75, 1.25, (B, C)).astype(np.float32)
        d = (2.0 * rng.integers(0, 2, (B, C)) + rng.uniform(-0.5, 0.5, (B, C))).astype(np.float32)
        aff = torch.from_numpy(np.stack([a, d], axis=-1)).cuda()
    xd = torch.from_numpy(x).cuda().to(DT[prec])
    raw, act = ops.fir_resample(xd, direction, affine=aff, want_raw=want_raw, want_act=want_act)
    torch.cuda.synchronize()
    assert (raw is not None) == want_raw and (act is not None) == (affine and want_act)
    n = fir_norm(direction)
    oshape = (B, 2 * H, 2 * W, C) if direction > 0 else (B, H // 2, W // 2, C)
    tag = f"fir[{name},{prec}]"
    line = f"{tag:60s} variant={variant_name(got_variant)}"
    if want_raw:
        assert tuple(raw.shape) == oshape
        got = raw.float().cpu().numpy()

        def raw_clip(b):
            exact = fir_scaled(x[b].astype(np.int32), direction, (0, 1))
            want = (exact / n).astype(np.float32)
            # the premise: the exact result is representable in the storage type (|64 ref| <= 128: 8 significant bits)
            assert np.array_equal(want.astype(np.float64) * n, exact)
            assert prec == "fp32" or np.array_equal(O.round_bf16(want), want)
            return int(np.count_nonzero(got[b] != want)), float(np.abs(got[b] - want).max())

        res = _per_clip(raw_clip, B)
        bad, maxdiff = sum(r[0] for r in res), max(r[1] for r in res)
        line += f" raw: mismatches={bad} maxdiff={maxdiff:.3e} tol=exact"
        del got
    else:
        bad = 0
    worst = e2 = 0.0
    tol = 4e-3 if prec == "bf16" else 2e-6
    if act is not None:
        assert tuple(act.shape) == oshape
        got = act.float().cpu().numpy()

        def act_clip(b):
            ref, bound = act_reference(x[b], a[b], d[b], direction, prec == "bf16")
            err = np.abs(got[b].astype(np.float64) - ref)
            i = np.unravel_index(np.argmax(err / bound), err.shape)
            return float(err[i] / bound[i]), (b,) + tuple(int(v) for v in i), float(err[i]), float(bound[i]), float((err ** 2).sum()), float((ref ** 2).sum())

        res = _per_clip(act_clip, B)
        w = max(res, key=lambda r: r[0])
        worst = w[0]
        e2 = float(np.sqrt(sum(r[4] for r in res) / sum(r[5] for r in res)))
        line += f" act: err={e2:.3e} tol={tol:.1e} worst/bound={worst:.3f}"
    ok = bad == 0 and worst <= 1.0 and e2 < tol
    report_line(line + (" OK" if ok else " FAIL"))
    assert bad == 0, f"{tag}: {bad} raw outputs differ from the exact result (max |diff| {maxdiff:.3e}), variant {got_variant}"
    if act is not None:
        assert e2 < tol, f"{tag}: activated output rel err {e2:.3e} >= {tol:.1e}"
        assert worst <= 1.0, f"{tag}: activated output |got - ref| = {w[2]:.3e} > bound {w[3]:.3e} at (b, y, x, c) = {w[1]}, variant {got_variant}"


def test_fir_march_float32_batch_independent(ops):
    """The float32 instantiation of the marching kernel (test_fir_down_marching_strips_bit_identical runs bf16 only): clip by clip the bits
    of the one-clip launches, which run other variants (4-row strips for one 768 x 256 clip, 4x1 blocks for one 384 x 128 clip)."""
    g = torch.Generator(device="cuda").manual_seed(11)
    for B, H, W, big, one in ((8, 768, 256, ("DOWN_MARCH", 16, 4, 4, 1, 1), ("DOWN_MARCH", 4, 4, 4, 1, 1)),
                              (8, 376, 132, ("DOWN_MARCH", 8, 4, 4, 1, 0), ("DOWN", 4, 1, 4, 1, 0))):
        C = 256
        assert ops.fir_variant(B, H, W, C, -1, torch.float32, affine=True) == big
        assert ops.fir_variant(1, H, W, C, -1, torch.float32, affine=True) == one
        x = torch.randn(B, H, W, C, device="cuda", generator=g)
        aff = torch.stack([1 + 0.2 * torch.randn(B, C, device="cuda", generator=g), 0.3 * torch.randn(B, C, device="cuda", generator=g)], -1).contiguous()
        raw, act = ops.fir_resample(x, -1, affine=aff)
        for b in (0, 3, B - 1):
            raw1, act1 = ops.fir_resample(x[b:b + 1].contiguous(), -1, affine=aff[b:b + 1].contiguous())
            assert torch.equal(raw[b], raw1[0]) and torch.equal(act[b], act1[0]), f"clip {b} of {B} x {H} x {W}"
        report_line(f"{'fir_march_fp32_batch_independent[' + str(H) + 'x' + str(W) + ']':60s} variant={variant_name(big)} vs {variant_name(one)} bit-identical OK")


def test_fir_variant_refusals(ops):
    """fd_fir_variant refuses what fd_fir_resample refuses, with the same error code."""
    from flowdec_amd import _lib as L
    lib = L.load()
    x = torch.zeros(1, 3, 4, 8, device="cuda")
    with pytest.raises(RuntimeError):
        ops.fir_resample(x, -1)                                                  # odd H in the down direction
    assert lib.fd_fir_variant(1, 3, 4, 8, -1, L.FD_F32, 0, 1, 0) == -1
    with pytest.raises(RuntimeError):
        ops.fir_resample(torch.zeros(1, 4, 4, 6, device="cuda"), 1)              # C % 4 != 0
    assert lib.fd_fir_variant(1, 4, 4, 6, 1, L.FD_F32, 0, 1, 0) == -1
