"""Exact-arithmetic data for the four Winograd convolution kernels (conv_wino.hip, conv_wino4.hip, conv_wino4f.hip, conv_wino44f.hip),
shared by test_wino_exact_cpu.py (no GPU: the premises and the teeth of the method) and test_hip_wino_exact.py (the kernels).

The data class.  G of F(4,3) has the entries 1/4, 1/6, 1/12, 1/24, so the weights lie on a 24 q grid: w = 24 q g with g in {-1, 0, 1}
and q = 2^-(6 + cout % 5) per output channel.  U = G w is then an integer multiple of q with |U| <= 24 q, the true divisions of the
pack kernels and the per-cout power-of-two scaling are exact, and with integer activations every product U V and every partial sum
is an integer multiple of q: below 2^24 quanta the float32 result EQUALS the float64 convolution whatever the order of summation.
F(2,3) (G = 1, 1/2) needs even multiples only.  The 2-D form F(4x4, 3x3) needs G g G^T: denominators up to 576 = 2^6 * 9, so its cases
draw g in {-3, 0, 3} (w = 72 q g'), which makes U an integer multiple of q / 8.

The fused GroupNorm + SiLU is exact too: fd_silu(u) = u * rcp(1 + __expf(-u)), and for u >= 17 the sum 1 + e^-u rounds to 1 in
float32 (e^-17 = 4.1e-8 < 2^-24), so silu(u) == u.  With integer x in [-2, 2], a in {1, 2} and integer d in [21, 24] the activated
operand is the integer a x + d in [17, 28].  The zero padding is applied AFTER the activation: padding zeroed before it would add
silu(d) ~ 24 per tap at every image border.

Every case has all-zero 3x3 rows (ZERO_ROWS: the m == 0 branch of the scale kernels), five different per-cout scales, bias rows on the
q grid, integer residuals |skip| <= 64 and 1x1 shortcut weights that are small multiples of q.  The 3x3 weights of every cout are
balanced (|sum g| <= G_SUM_MAX), which keeps sum |y| over a 16 x 16 tile below 2^24 quanta: the statistics output is exact too."""
import functools
import types
import zlib

import numpy as np

BT4 = np.array([[4, 0, -5, 0, 1, 0], [0, -4, -4, 1, 1, 0], [0, 4, -4, -1, 1, 0], [0, -2, -1, 2, 1, 0], [0, 2, -1, -2, 1, 0],
                [0, 4, 0, -5, 0, 1]], np.float64)
G24 = np.array([[6, 0, 0], [-4, -4, -4], [-4, 4, -4], [1, 2, 4], [1, -2, 4], [0, 0, 24]], np.float64)      # 24 G of F(4,3)
AT4 = np.array([[1, 1, 1, 1, 1, 0], [0, 1, -1, 2, -2, 0], [0, 1, 1, 4, 4, 0], [0, 1, -1, 8, -8, 1]], np.float64)
BT2 = np.array([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]], np.float64)
G2 = np.array([[2, 0, 0], [1, 1, 1], [1, -1, 1], [0, 0, 2]], np.float64)                                   # 2 G of F(2,3)
AT2 = np.array([[1, 1, 1, 0], [0, 1, -1, -1]], np.float64)

KERNELS = {"WINO": ("bf16", True, "f23"), "WINO4": ("bf16", 4, "f43"), "WINO4F": ("fp32", 4, "f43"), "WINO44F": ("fp32", 44, "f44")}


G_SUM_MAX = 30    # |sum of a cout's 3x3 weights| in units of 24 q: 256 x 24 x 22.5 x 30 = 0.25 x 2^24 quanta of sum |y| per tile


def zero_rows(Cout):
    """Couts whose 3x3 weights are all zero: one in the first cout block (its shortcut weights are zero too), one in the last."""
    return (7, Cout - 3)


# ---------------------------------------------------------------------------------------------------------
# the cases.  (name, B, H, W, C0, C1, Cout, act, bias_rows ("B" = one row per image), skip, scale, S0, S1, density of the 3x3 weights)
# ---------------------------------------------------------------------------------------------------------
def _c(name, B, H, W, C0, C1, act, rows, skip, scale, S0=0, S1=0, Cout=256, density=1.0):
    return (name, B, H, W, C0, C1, Cout, act, rows, skip, scale, S0, S1, density)


# F(4,3) bf16 (channels % 32, whole 16 x 16 tiles, C0 + C1 <= 512).  Images: one tile (four borders), one neighbour in W / in H, one
# interior tile (48 x 48), grids of 3 (< 8: the XCD remap's short tail), 27 and 18 blocks.  Channels: 32 = one chunk pair (ring run-in
# == run-out), 64, 96 (odd pair count), 32+32 (segment switch at the first pair), 256+64, 480+32 and 256+256 (the affine limit).
# Every instantiation <ACT, SKIP, SC>: (raw / act) x (plain / skip / sc); bias rows 0, 1, B; scale 1 and 1/2.
WINO4_CASES = [
    _c("t1_c32_raw_plain", 1, 16, 16, 32, 0, False, 0, False, 1.0),
    _c("t1_c32_act_skip", 1, 16, 16, 32, 0, True, 1, True, 0.5),
    _c("t1_c64_act_plain", 1, 16, 16, 64, 0, True, 0, False, 0.5),
    _c("t1_c96_raw_skip", 1, 16, 16, 96, 0, False, 1, True, 1.0),
    _c("w2_c64_act_plain", 1, 16, 32, 64, 0, True, 1, False, 1.0),
    _c("w2_c32_32_raw_skip", 1, 16, 32, 32, 32, False, 1, True, 0.5),
    _c("h2_c64_raw_skip", 1, 32, 16, 64, 0, False, "B", True, 0.5),
    _c("h2_c96_act_plain", 1, 32, 16, 96, 0, True, 1, False, 0.5),
    _c("i9_c96_act_skip", 1, 48, 48, 96, 0, True, 1, True, 1.0),
    _c("i9_c32_raw_plain", 1, 48, 48, 32, 0, False, 1, False, 0.5),
    _c("i9_c32_32_act_skip", 1, 48, 48, 32, 32, True, 0, True, 0.5),
    _c("g3_c32_32_act_plain", 3, 16, 16, 32, 32, True, "B", False, 0.5),
    _c("g3_c64_raw_skip", 3, 16, 16, 64, 0, False, "B", True, 1.0),
    _c("g27_c64_act_skip", 3, 48, 48, 64, 0, True, "B", True, 0.5),
    _c("g27_c96_raw_plain", 3, 48, 48, 96, 0, False, 1, False, 1.0),
    _c("g18_c32_act_skip", 9, 16, 32, 32, 0, True, "B", True, 1.0),
    _c("g18_c64_act_plain", 9, 16, 32, 64, 0, True, 1, False, 0.5),
    _c("w2_c256_64_act_skip", 1, 16, 32, 256, 64, True, 1, True, 0.5),
    _c("w2_c256_64_raw_plain", 1, 16, 32, 256, 64, False, 0, False, 1.0),
    _c("w2_c480_32_act_plain", 1, 16, 32, 480, 32, True, 1, False, 1.0),
    _c("t1_c256_256_act_skip", 1, 16, 16, 256, 256, True, 1, True, 0.5),
    _c("w2_c256_256_raw_skip", 1, 16, 32, 256, 256, False, 0, True, 1.0),
    _c("g3_c256_256_act_plain", 3, 16, 16, 256, 256, True, "B", False, 1.0),
    _c("t1_c32_raw_sc32", 1, 16, 16, 32, 0, False, 1, False, 1.0, S0=32),
    _c("g3_c64_act_sc32", 3, 16, 16, 64, 0, True, "B", False, 0.5, S0=32),
    _c("w2_c96_act_sc64_32", 1, 16, 32, 96, 0, True, 1, False, 1.0, S0=64, S1=32),
    _c("h2_c32_32_raw_sc64_32", 1, 32, 16, 32, 32, False, 0, False, 0.5, S0=64, S1=32),
    _c("w2_c32_32_act_sc256_256", 1, 16, 32, 32, 32, True, 1, False, 0.5, S0=256, S1=256),
    _c("t1_c256_256_raw_sc256_256", 1, 16, 16, 256, 256, False, 0, False, 1.0, S0=256, S1=256),
    _c("t1_c480_32_act_sc32", 1, 16, 16, 480, 32, True, 1, False, 0.5, S0=32),
    _c("i9_c64_act_sc32", 1, 48, 48, 64, 0, True, 1, False, 1.0, S0=32),
    _c("g27_c32_raw_sc32", 3, 48, 48, 32, 0, False, "B", False, 1.0, S0=32),
    _c("g18_c64_raw_sc64_32", 9, 16, 32, 64, 0, False, "B", False, 0.5, S0=64, S1=32),
    _c("g18_c96_act_sc32", 9, 16, 32, 96, 0, True, "B", False, 1.0, S0=32),
    _c("h2_c256_256_act_sc32", 1, 32, 16, 256, 256, True, 1, False, 1.0, S0=32),
    _c("g3_c96_raw_plain", 3, 16, 16, 96, 0, False, 0, False, 0.5),
    _c("i9_c256_64_act_plain", 1, 48, 48, 256, 64, True, "B", False, 0.5),
    _c("g18_c32_32_raw_skip", 9, 16, 32, 32, 32, False, "B", True, 1.0),
]

# F(4,3) f32 (channels % 16): a subset of the above plus 16, 48, 16+16 and shortcut 16 (one / three / 1+1 chunk pairs of 8-channel chunks)
WINO4F_CASES = [
    _c("t1_c16_raw_plain", 1, 16, 16, 16, 0, False, 0, False, 1.0),
    _c("t1_c16_act_skip", 1, 16, 16, 16, 0, True, 1, True, 0.5),
    _c("w2_c48_act_plain", 1, 16, 32, 48, 0, True, 1, False, 0.5),
    _c("h2_c48_raw_skip", 1, 32, 16, 48, 0, False, "B", True, 1.0),
    _c("t1_c16_16_act_plain", 1, 16, 16, 16, 16, True, 0, False, 1.0),
    _c("g3_c16_16_raw_skip", 3, 16, 16, 16, 16, False, "B", True, 0.5),
    _c("i9_c32_act_skip", 1, 48, 48, 32, 0, True, 1, True, 1.0),
    _c("i9_c48_raw_plain", 1, 48, 48, 48, 0, False, 1, False, 0.5),
    _c("g27_c64_act_skip", 3, 48, 48, 64, 0, True, "B", True, 0.5),
    _c("g18_c32_act_plain", 9, 16, 32, 32, 0, True, "B", False, 1.0),
    _c("g18_c16_raw_skip", 9, 16, 32, 16, 0, False, 1, True, 0.5),
    _c("w2_c256_64_act_skip", 1, 16, 32, 256, 64, True, 1, True, 0.5),
    _c("w2_c480_32_act_plain", 1, 16, 32, 480, 32, True, 1, False, 1.0),
    _c("t1_c256_256_act_skip", 1, 16, 16, 256, 256, True, 1, True, 0.5),
    _c("w2_c256_256_raw_plain", 1, 16, 32, 256, 256, False, 0, False, 1.0),
    _c("t1_c16_raw_sc16", 1, 16, 16, 16, 0, False, 1, False, 1.0, S0=16),
    _c("g3_c48_act_sc16", 3, 16, 16, 48, 0, True, "B", False, 0.5, S0=16),
    _c("w2_c96_act_sc64_32", 1, 16, 32, 96, 0, True, 1, False, 1.0, S0=64, S1=32),
    _c("h2_c16_16_raw_sc64_32", 1, 32, 16, 16, 16, False, 0, False, 0.5, S0=64, S1=32),
    _c("w2_c32_32_act_sc256_256", 1, 16, 32, 32, 32, True, 1, False, 0.5, S0=256, S1=256),
    _c("t1_c256_256_raw_sc256_256", 1, 16, 16, 256, 256, False, 0, False, 1.0, S0=256, S1=256),
    _c("i9_c64_act_sc32", 1, 48, 48, 64, 0, True, 1, False, 1.0, S0=32),
    _c("g18_c64_raw_sc16", 9, 16, 32, 64, 0, False, "B", False, 0.5, S0=16),
    _c("g27_c16_act_sc16", 3, 48, 48, 16, 0, True, "B", False, 1.0, S0=16),
    _c("g3_c16_act_plain", 3, 16, 16, 16, 0, True, 1, False, 0.5),
    _c("h2_c16_16_act_skip", 1, 32, 16, 16, 16, True, "B", True, 1.0),
    _c("i9_c16_16_raw_sc16", 1, 48, 48, 16, 16, False, 0, False, 1.0, S0=16),
    _c("w2_c48_raw_sc16", 1, 16, 32, 48, 0, False, 1, False, 0.5, S0=16),
]

# 2-D F(4x4, 3x3) f32 (channels % 8, Cout % 128; shortcut and residual together).  U lives on a q / 8 grid, 576 times finer than the
# weights: the wide cases thin the weights (density) until the partial-sum bound is below 2^24 (test_wino_exact_cpu.py asserts it; they
# sit at 0.8 - 0.9 of it).  At 512 channels that is a density of 1/16 - 1/32, about 1.5 non-zero weights per cout and 8-channel chunk:
# one cout alone would miss most defects of a single chunk, the 128 - 384 couts of a case together see every (chunk, tap).
WINO44F_CASES = [
    _c("t1_c8_raw_plain_o128", 1, 16, 16, 8, 0, False, 0, False, 1.0, Cout=128),
    _c("t1_c8_act_skip_o128", 1, 16, 16, 8, 0, True, 1, True, 0.5, Cout=128),
    _c("t1_c24_act_plain", 1, 16, 16, 24, 0, True, 1, False, 0.5),
    _c("w2_c24_raw_skip_o384", 1, 16, 32, 24, 0, False, "B", True, 1.0, Cout=384),
    _c("h2_c8_8_act_skip", 1, 32, 16, 8, 8, True, 0, True, 1.0),
    _c("g3_c8_8_raw_plain_o384", 3, 16, 16, 8, 8, False, "B", False, 0.5, Cout=384),
    _c("i9_c24_act_skip_o128", 1, 48, 48, 24, 0, True, 1, True, 0.5, Cout=128),
    _c("i9_c8_8_raw_plain", 1, 48, 48, 8, 8, False, 1, False, 1.0),
    _c("g27_c24_act_skip_o384", 3, 48, 48, 24, 0, True, "B", True, 0.5, Cout=384),
    _c("g18_c8_act_plain", 9, 16, 32, 8, 0, True, "B", False, 1.0),
    _c("g18_c64_raw_skip_o128", 9, 16, 32, 64, 0, False, 1, True, 0.5, Cout=128),
    _c("w2_c64_act_plain_o384", 1, 16, 32, 64, 0, True, 1, False, 1.0, Cout=384, density=1 / 4),
    _c("t1_c256_256_act_skip", 1, 16, 16, 256, 256, True, 1, True, 0.5, density=1 / 32),
    _c("w2_c256_256_raw_plain_o128", 1, 16, 32, 256, 256, False, 0, False, 1.0, Cout=128, density=1 / 16),
    _c("g3_c256_256_act_plain_o384", 3, 16, 16, 256, 256, True, "B", False, 1.0, Cout=384, density=1 / 32),
    _c("t1_c8_raw_sc8_o128", 1, 16, 16, 8, 0, False, 1, False, 1.0, S0=8, Cout=128),
    _c("t1_c24_act_sc8_skip", 1, 16, 16, 24, 0, True, 1, True, 0.5, S0=8),
    _c("w2_c8_8_act_sc64_8_skip_o384", 1, 16, 32, 8, 8, True, "B", True, 0.5, S0=64, S1=8, Cout=384),
    _c("h2_c64_raw_sc64_8", 1, 32, 16, 64, 0, False, 0, False, 1.0, S0=64, S1=8),
    _c("g3_c24_act_sc8_skip_o128", 3, 16, 16, 24, 0, True, "B", True, 1.0, S0=8, Cout=128),
    _c("i9_c64_act_sc64_8_skip", 1, 48, 48, 64, 0, True, 1, True, 0.5, S0=64, S1=8, density=1 / 4),
    _c("g27_c8_raw_sc8_o384", 3, 48, 48, 8, 0, False, "B", False, 0.5, S0=8, Cout=384),
    _c("g18_c24_act_sc64_8_skip", 9, 16, 32, 24, 0, True, "B", True, 1.0, S0=64, S1=8),
    _c("t1_c256_256_raw_sc64_8_skip", 1, 16, 16, 256, 256, False, 1, True, 0.5, S0=64, S1=8, density=1 / 16),
    _c("h2_c24_raw_plain_o128", 1, 32, 16, 24, 0, False, 1, False, 0.5, Cout=128),
    _c("w2_c8_act_sc8_o384", 1, 16, 32, 8, 0, True, 0, False, 1.0, S0=8, Cout=384),
    _c("g3_c64_act_skip", 3, 16, 16, 64, 0, True, "B", True, 1.0, density=1 / 4),
    _c("t1_c8_8_raw_skip_o384", 1, 16, 16, 8, 8, False, 1, True, 0.5, Cout=384),
]

# F(2,3) bf16 (channels % 32, Cout in {128, 256, 512}, ragged tiles allowed)
WINO_CASES = [
    _c("r20x13_c32_raw_plain_o128", 1, 20, 13, 32, 0, False, 0, False, 1.0, Cout=128),
    _c("r20x13_c32_act_skip_o128", 1, 20, 13, 32, 0, True, 1, True, 0.5, Cout=128),
    _c("r20x13_c64_32_act_plain", 1, 20, 13, 64, 32, True, 1, False, 0.5),
    _c("r20x13_c64_32_raw_skip_o512", 1, 20, 13, 64, 32, False, 1, True, 1.0, Cout=512),
    _c("t1_c32_act_plain_o128", 1, 16, 16, 32, 0, True, 1, False, 1.0, Cout=128),
    _c("t1_c256_256_act_skip", 1, 16, 16, 256, 256, True, 1, True, 0.5),
    _c("t1_c256_256_raw_plain_o128", 1, 16, 16, 256, 256, False, 0, False, 1.0, Cout=128),
    _c("g30_c32_act_skip", 2, 48, 80, 32, 0, True, "B", True, 0.5),
    _c("g30_c64_32_raw_skip_o128", 2, 48, 80, 64, 32, False, "B", True, 1.0, Cout=128),
    _c("g30_c64_32_act_plain_o512", 2, 48, 80, 64, 32, True, 1, False, 1.0, Cout=512),
    _c("t1_c32_raw_sc64_o128", 1, 16, 16, 32, 0, False, 1, False, 1.0, S0=64, Cout=128),
    _c("r20x13_c64_32_act_sc64", 1, 20, 13, 64, 32, True, 1, False, 0.5, S0=64),
    _c("r20x13_c32_act_sc128_256_skip_o128", 1, 20, 13, 32, 0, True, 1, True, 1.0, S0=128, S1=256, Cout=128),
    _c("t1_c256_256_act_sc128_256", 1, 16, 16, 256, 256, True, 1, False, 1.0, S0=128, S1=256),
    _c("g30_c32_act_sc64_o128", 2, 48, 80, 32, 0, True, "B", False, 0.5, S0=64, Cout=128),
    _c("g30_c64_32_raw_sc64_skip", 2, 48, 80, 64, 32, False, "B", True, 0.5, S0=64),
    _c("t1_c64_32_raw_skip", 1, 16, 16, 64, 32, False, "B", True, 0.5),
    _c("t1_c32_raw_skip_o512", 1, 16, 16, 32, 0, False, 1, True, 1.0, Cout=512),
    _c("r20x13_c256_256_act_skip_o128", 1, 20, 13, 256, 256, True, 1, True, 0.5, Cout=128),
    _c("r20x13_c32_raw_sc64_skip", 1, 20, 13, 32, 0, False, 0, True, 1.0, S0=64),
    _c("g30_c32_raw_plain_o512", 2, 48, 80, 32, 0, False, 0, False, 1.0, Cout=512),
    _c("t1_c64_32_act_sc128_256_o512", 1, 16, 16, 64, 32, True, 1, False, 0.5, S0=128, S1=256, Cout=512),
]

# batch independence (test_wino_batch_independent): per-image affine and bias rows
BATCH_CASES = {"WINO4": _c("batch_c64_act_skip", 3, 16, 32, 64, 0, True, "B", True, 0.5),
               "WINO44F": _c("batch_c24_act_sc8_skip", 3, 16, 32, 24, 0, True, "B", True, 0.5, S0=8, Cout=128)}

CASES = {"WINO": WINO_CASES, "WINO4": WINO4_CASES, "WINO4F": WINO4F_CASES, "WINO44F": WINO44F_CASES}
ALL_CASES = [(k, c) for k in ("WINO4", "WINO4F", "WINO44F", "WINO") for c in CASES[k]]
ALL_IDS = [f"{k}-{c[0]}" for k, c in ALL_CASES]


def conv64(x, w):
    """float64 convolution, stride 1, zero 'same' padding: x [B, Ci, H, W], w [Co, Ci, k, k]."""
    import torch
    k = w.shape[-1]
    return torch.nn.functional.conv2d(torch.from_numpy(np.ascontiguousarray(x, np.float64)), torch.from_numpy(np.ascontiguousarray(w, np.float64)),
                                      padding=k // 2).numpy()


@functools.lru_cache(maxsize=4)
def _make(kernel, case):
    name, B, H, W, C0, C1, Cout, act, rows, skip, scale, S0, S1, density = case
    rng = np.random.default_rng(zlib.crc32(f"wino_exact/{kernel}/{name}".encode()))
    c = types.SimpleNamespace(kernel=kernel, name=name, B=B, H=H, W=W, C0=C0, C1=C1, Cout=Cout, act=act, skip_on=skip, scale=scale, S0=S0, S1=S1)
    Cin = C0 + C1
    c.form = KERNELS[kernel][2]
    c.qexp = 6 + np.arange(Cout) % 5
    c.q = np.ldexp(1.0, -c.qexp)                                    # per-cout quantum
    c.gmul = 3 if c.form == "f44" else 1                            # G g G^T needs g divisible by 3
    c.x = rng.integers(-2, 3, (B, Cin, H, W)).astype(np.float64)
    g = rng.integers(-1, 2, (Cout, Cin, 3, 3))
    if density < 1.0:
        g = g * (rng.random(g.shape) < density)
    g[list(zero_rows(Cout))] = 0
    # Balance every cout row: with the activation the operand is d ~ 22 plus a small signed part, so an output is about 24 q x 22 x sum g,
    # and over the 256 pixels of a tile sum |y| would pass 2^24 quanta for the rows whose weights happen to sum to more than ~100 (the
    # statistics output could then not be exact).  Flip surplus weights of the majority sign until |sum g| <= G_SUM_MAX.
    for o in range(Cout):
        s = int(g[o].sum())
        if abs(s) * c.gmul > G_SUM_MAX:
            flat = g[o].reshape(-1)
            surplus = rng.permutation(np.flatnonzero(flat == np.sign(s)))[:-(-(abs(s) - G_SUM_MAX // c.gmul) // 2)]
            flat[surplus] = -np.sign(s)
    c.g = (g * c.gmul).astype(np.float64)                           # w = 24 q g
    c.w = 24.0 * c.q[:, None, None, None] * c.g
    c.a = c.d = None
    z = c.x
    if act:
        c.a = rng.choice([1.0, 2.0], (B, Cin))
        c.d = rng.integers(21, 25, (B, Cin)).astype(np.float64)
        z = c.x * c.a[:, :, None, None] + c.d[:, :, None, None]     # = silu of itself in float32: an integer in [17, 28]
    c.z = z
    ref = conv64(z, c.w)                                            # zero padding AFTER the activation
    c.xs = c.ms = c.ws = None
    if S0:
        c.xs = rng.integers(-2, 3, (B, S0 + S1, H, W)).astype(np.float64)
        c.ms = rng.integers(-2, 3, (Cout, S0 + S1)).astype(np.float64) * (18 if c.form == "f44" else 1)   # 2-D: (1/6)^2 = 16 / 576 of it must be on the q / 8 grid
        c.ms[zero_rows(Cout)[0]] = 0
        c.ws = c.ms * c.q[:, None]
        ref = ref + np.einsum("os,bshw->bohw", c.ws, c.xs)
    c.bias_rows = B if rows == "B" else rows
    c.bias = None
    if c.bias_rows:
        c.bias = rng.integers(-8, 9, (c.bias_rows, Cout)) * c.q[None, :]
        ref = ref + c.bias[:, :, None, None]
    c.skip = None
    if skip:
        c.skip = rng.integers(-64, 65, (B, Cout, H, W)).astype(np.float64)
        ref = ref + c.skip
    c.ref = ref * scale
    c.ref.setflags(write=False)
    return c


def make_case(kernel, case):
    """The tensors of one case (NCHW float64: x, w, a, d, xs, ws, bias, skip; all exactly representable in bf16 / fp16 / f32 as needed)
    and c.ref, the float64 result scale * (conv3x3(act(x)) + conv1x1(xs) + bias + skip)."""
    return _make(kernel, tuple(case))


def exact_in_f32(a):
    return bool(np.array_equal(np.asarray(a, np.float64).astype(np.float32).astype(np.float64), a))


def mismatches(got, ref, storage):
    """Indices (b, cout, h, w) at which `got` is not THE correctly stored exact result (bf16: after the one rounding of the store)."""
    want = ref
    if storage == "bf16":
        from oracle import flowdec_oracle as O
        want = O.round_bf16(np.asarray(ref, np.float32)).astype(np.float64)
    return np.argwhere(np.asarray(got, np.float64) != want)


def describe_mismatches(idx, c):
    """Where the mismatches are: the first coordinates, how many in border tiles, in the last cout block, and per position w % 4."""
    if len(idx) == 0:
        return ""
    th, tw = -(-c.H // 16), -(-c.W // 16)
    ti, tj = idx[:, 2] // 16, idx[:, 3] // 16
    border = int(np.count_nonzero((ti == 0) | (ti == th - 1) | (tj == 0) | (tj == tw - 1)))
    last_blk = int(np.count_nonzero(idx[:, 1] >= c.Cout - 128))
    per_w = [int(np.count_nonzero(idx[:, 3] % 4 == r)) for r in range(4)]
    return (f" first(b,cout,h,w)={[tuple(int(v) for v in r) for r in idx[:4]]} border_tiles={border} last_cout_block={last_blk} "
            f"w%4={per_w} couts={len(np.unique(idx[:, 1]))}")


# ---------------------------------------------------------------------------------------------------------
# the premises, in integers
# ---------------------------------------------------------------------------------------------------------
def _padded(z, Wp=None):
    B, C, H, W = z.shape
    Wp = W if Wp is None else Wp
    zp = np.zeros((B, C, H + 2, Wp + 2))
    zp[:, :, 1:H + 1, 1:W + 1] = z
    return zp


def _windows_w(zp, m):
    """zp [B, C, H + 2, W + 2] -> [B, C, H + 2, W / m, m + 2]: the input window of every 1 x m output tile."""
    return np.lib.stride_tricks.sliding_window_view(zp, m + 2, axis=3)[:, :, :, ::m, :]


def premise(c, form=None):
    """max |V| of the transformed input and the largest partial-sum bound sum_xi |A^T| sum |U| |V| (+ shortcut, bias, residual) over all
    outputs, in quanta of the output's own cout (q for the 1-D forms, q / 8 for the 2-D form).  The bound covers ANY partial sum of the
    kernel's arithmetic in ANY order; below 2^24 every float32 operation on these integers is exact."""
    form = form or c.form
    B, Cin, H, W = c.z.shape
    extra = np.zeros((B, c.Cout, H, W))
    if c.ws is not None and form != "f44":
        # conv_wino4(f).hip: a direct GEMM on the output planes; conv_wino.hip: M0 += W x(y0), M3 -= W x(y1), M1 / M2 += W/2 (x(y0) +- x(y1)),
        # so that a partial sum of y0 or y1 holds at most |W| (2 |x(y0)| + |x(y1)|) <= 3 |W| max |x|
        extra += (3.0 if form == "f23" else 1.0) * np.einsum("os,bshw->bohw", np.abs(c.ms), np.abs(c.xs))
    if c.bias is not None:
        extra += np.abs(c.bias / c.q[None, :])[np.arange(B) % c.bias_rows][:, :, None, None]
    if c.skip is not None:
        extra += np.abs(c.skip) * np.ldexp(1.0, c.qexp)[None, :, None, None]
    if form in ("f23", "f43"):
        m, BT, Gn, AT = (2, BT2, 12.0 * G2, AT2) if form == "f23" else (4, BT4, G24, AT4)
        Wp = -(-W // m) * m
        V = np.abs(_windows_w(_padded(c.z, Wp), m) @ BT.T)                    # [B, C, H + 2, nt, P]
        vmax = float(V.max())
        V = np.ascontiguousarray(np.moveaxis(V, -1, 0))                       # [P, B, C, H + 2, nt]
        U = np.abs(np.einsum("xk,ocdk->ocdx", Gn, c.g))                       # units of q: U = G (24 q g)
        P, nt = BT.shape[0], Wp // m
        S = np.zeros((B, c.Cout, H, nt, P))
        for b in range(B):
            for xi in range(P):
                for dy in range(3):
                    S[b, :, :, :, xi] += (np.ascontiguousarray(U[:, :, dy, xi]) @ V[xi, b, :, dy:dy + H].reshape(Cin, -1)).reshape(c.Cout, H, nt)
        bound = np.einsum("yx,bohtx->bohty", np.abs(AT), S).reshape(B, c.Cout, H, Wp)[:, :, :, :W] + extra
        return vmax, float(bound.max())
    assert form == "f44" and H % 4 == 0 and W % 4 == 0
    zp = _padded(c.z)
    D = np.lib.stride_tricks.sliding_window_view(zp, (6, 6), axis=(2, 3))[:, :, ::4, ::4]       # [B, C, H/4, W/4, 6, 6]
    V = np.abs(BT4 @ D @ BT4.T)
    U = np.abs(np.einsum("ia,ocab,jb->ocij", G24, c.g, G24)) / 3.0                              # units of q / 8: U = G (24 q g) G^T
    S = np.zeros((B, c.Cout, H // 4, W // 4, 6, 6))
    for b in range(B):
        for i in range(6):
            for j in range(6):
                S[b, :, :, :, i, j] = (U[:, :, i, j] @ V[b, :, :, :, i, j].reshape(Cin, -1)).reshape(c.Cout, H // 4, W // 4)
    if c.ws is not None:   # the shortcut as centre-tap chunks in the Winograd domain: U = G[:, 1] G[:, 1]^T w on the 16 inner positions
        Ds = np.lib.stride_tricks.sliding_window_view(_padded(c.xs), (6, 6), axis=(2, 3))[:, :, ::4, ::4]
        Vs = np.abs(BT4 @ Ds @ BT4.T)
        Us = np.abs(np.einsum("i,os,j->osij", G24[:, 1], c.ms, G24[:, 1])) / 72.0
        for b in range(B):
            for i in range(1, 5):
                for j in range(1, 5):
                    S[b, :, :, :, i, j] += (Us[:, :, i, j] @ Vs[b, :, :, :, i, j].reshape(Vs.shape[1], -1)).reshape(c.Cout, H // 4, W // 4)
    A = np.abs(AT4)
    bound = np.einsum("yi,bohtij,xj->bohytx", A, S, A).reshape(B, c.Cout, H, W) + 8.0 * extra
    return float(V.max()), float(bound.max())


# ---------------------------------------------------------------------------------------------------------
# emulations of the kernels' arithmetic
# ---------------------------------------------------------------------------------------------------------
MUTATIONS = ("drop_tap", "pad_before_act", "neighbour_scale", "skip_last_chunk")


def emulate_f43(c, mutation=None, chunk=16, U_EXP=9):
    """conv_wino4.hip's arithmetic on a case (F(4,3) along W x direct along H, per-cout power-of-two weight scale, fp16 operands,
    16-channel chunks, the folded shortcut in the same accumulators, out = acc (scale / wscale) + skip scale + bias scale), in float64:
    every value is an integer multiple of q far below 2^53, so float64 is exact here and any f32 / fp16 rounding the kernel would do is
    asserted away.  `mutation` plants one defect of the kind the relative-L2 tolerances cannot see."""
    B, Cin, H, W = c.z.shape
    assert W % 4 == 0
    w = c.w.copy()
    if mutation == "drop_tap":
        ch, dy, dx = np.argwhere(w[9] != 0)[len(w[9].ravel()) // 40]      # one (tap, channel) of one cout (q = 2^-10)
        w[9, ch, dy, dx] = 0.0
    if mutation == "pad_before_act" and c.act:
        zp = _padded(c.x) * c.a[:, :, None, None] + c.d[:, :, None, None]    # the padding went through silu(a 0 + d) = d
    else:
        zp = _padded(c.z)
    U = np.einsum("xk,ocdk->ocdx", G24, w / 24.0)                        # G w: the divisions are exact on the 24 q grid
    m = np.abs(U).max(axis=(1, 2, 3))
    k = np.where(m > 0, U_EXP - np.frexp(np.where(m > 0, m, 1.0))[1], 0)  # wino4_scale_kernel: m 2^k in [2^(U_EXP-1), 2^U_EXP)
    Us = U * np.ldexp(1.0, k)[:, None, None, None]
    V = _windows_w(zp, 4) @ BT4.T                                        # [B, C, H + 2, nt, 6]
    assert np.array_equal(Us.astype(np.float16).astype(np.float64), Us) and np.array_equal(V.astype(np.float16).astype(np.float64), V)
    nt = W // 4
    M = np.zeros((B, c.Cout, H, nt, 6))
    for c0 in range(0, Cin, chunk):
        couts = slice(0, c.Cout - 128) if mutation == "skip_last_chunk" and c0 + chunk >= Cin else slice(0, c.Cout)   # the last cout block misses it
        for b in range(B):
            for xi in range(6):
                for dy in range(3):
                    M[b, couts, :, :, xi] += (Us[couts, c0:c0 + chunk, dy, xi] @ V[b, c0:c0 + chunk, dy:dy + H, :, xi].reshape(chunk, -1)).reshape(-1, H, nt)
    y = np.einsum("yx,bohtx->bohty", AT4, M).reshape(B, c.Cout, H, W)
    if c.ws is not None:
        y = y + np.einsum("os,bshw->bohw", c.ws * np.ldexp(1.0, k)[:, None], c.xs)
    inv = np.ldexp(1.0, -k)
    if mutation == "neighbour_scale":
        inv = np.roll(inv, -1)                                           # cout c reads the table row of cout c + 1
    out = y * (inv * c.scale)[None, :, None, None]
    if c.skip is not None:
        out = out + c.skip * c.scale
    if c.bias is not None:
        out = out + (c.bias * c.scale)[np.arange(B) % c.bias_rows][:, :, None, None]
    return out


def emulate_f44_f32(c):
    """conv_wino44f.hip in float32 NumPy: U = G g G^T as its pack kernel computes it (integer numerators 24 G in double, one division by
    576, one rounding to float32), V = B^T d B, sequential float32 accumulation over the channels (product rounded, then the sum), the
    shortcut as centre-tap chunks, Y = A^T M A, then ((Y + bias) + skip) scale.  Returns the float32 result."""
    f = np.float32
    B, Cin, H, W = c.z.shape
    U = (np.einsum("ia,ocab,jb->ocij", G24, c.w.astype(f).astype(np.float64), G24) / 576.0).astype(f)
    D = np.lib.stride_tricks.sliding_window_view(_padded(c.z), (6, 6), axis=(2, 3))[:, :, ::4, ::4]
    V = (BT4 @ D @ BT4.T).astype(f)                                      # integers: exact
    M = np.zeros((B, c.Cout, H // 4, W // 4, 6, 6), f)
    for ch in range(Cin):
        M += (U[None, :, ch, None, None] * V[:, None, ch]).astype(f)
    if c.ws is not None:
        Ds = np.lib.stride_tricks.sliding_window_view(_padded(c.xs), (6, 6), axis=(2, 3))[:, :, ::4, ::4]
        Vs = (BT4 @ Ds @ BT4.T).astype(f)
        Gc = G24[:, 1]
        Usc = (np.einsum("i,os,j->osij", Gc, c.ws.astype(f).astype(np.float64), Gc) / 576.0).astype(f)
        for ch in range(c.ws.shape[1]):
            M += (Usc[None, :, ch, None, None] * Vs[:, None, ch]).astype(f)
    A = AT4.astype(f)
    T = np.einsum("yi,bohtij->bohtyj", A, M).astype(f)
    Y = np.einsum("bohtyj,xj->bohytx", T, A).astype(f).reshape(B, c.Cout, H, W)
    if c.bias is not None:
        Y = Y + c.bias.astype(f)[np.arange(B) % c.bias_rows][:, :, None, None]
    if c.skip is not None:
        Y = Y + c.skip.astype(f)
    return (Y * f(c.scale)).astype(f)


def tile_sums(ref, power):
    """Exact per-(image, 16 x 16 tile, cout) sums of ref^power: [B, tiles, Cout], tiles in row-major order (fd_conv_stats_tiles)."""
    B, Co, H, W = ref.shape
    th, tw = -(-H // 16), -(-W // 16)
    r = np.zeros((B, Co, th * 16, tw * 16))
    r[:, :, :H, :W] = ref ** power
    return r.reshape(B, Co, th, 16, tw, 16).sum(axis=(3, 5)).reshape(B, Co, th * tw).transpose(0, 2, 1)
