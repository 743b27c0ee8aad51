"""References, data and error bounds of the operator-level solver tests (tests/test_hip_solver_ops.py on the GPU, tests/test_solver_ops_cpu.py
without one; include/flowdec_hip.h "Operator-level: solver and edge kernels").

Three things per kernel:
  *_ref   the operation in NumPy float64, computed from the stored inputs (the float32 / bf16 values the kernel reads);
  *_bound the per-element error bound, derived from the kernel's operation count with u = 2^-24 (first order in u: a chain of m float32
          roundings on a term of magnitude a contributes at most m u a; the derivation is in each function's docstring);
  *_f32   a float32 restatement of the kernel's formula, once with every product-sum fused (float64 product and sum, rounded once) and
          once unfused (product rounded, then the sum) -- the compiler may contract a multiply-add or not, and a bound has to hold in
          both cases.  The CPU tests run the restatements against the bounds, so that a bound is a condition the arithmetic itself meets.

Complex planes are float32 arrays with a trailing axis of 2 (re, im): every kernel but the error norm treats the two components alike.
"""
import ctypes as C

import numpy as np
import torch

U = 2.0 ** -24          # unit roundoff of float32
U_BF16 = 2.0 ** -8      # unit roundoff of bfloat16 (8 significand bits)
F64 = np.float64
NAN_BITS = -1           # int32 0xffffffff: a NaN no kernel here produces (the sentinel of unwritten outputs)


# ---- number formats ---------------------------------------------------------------------------------------------------------------
def f32(a):
    return np.asarray(a, F64).astype(np.float32)


def stored(a, dtype):
    """The float32 array `a` as a tensor of `dtype` holds it (bf16: round to nearest even), back in float32."""
    a = np.ascontiguousarray(a, np.float32)
    return a if dtype == "fp32" else torch.from_numpy(a).to(torch.bfloat16).float().numpy()


def mul32(a, b):
    return f32(np.asarray(a, F64) * np.asarray(b, F64))


def add32(a, b):
    return f32(np.asarray(a, F64) + np.asarray(b, F64))


def fma32(a, b, c, fused):
    """a * b + c on float32 operands: the float64 product is exact (24 x 24 bits); fused rounds the sum once, unfused the product first."""
    p = np.asarray(a, F64) * np.asarray(b, F64)
    return f32(p + np.asarray(c, F64)) if fused else add32(f32(p), c)


def sentinel(shape):
    """float32 array of NaNs with the bit pattern NAN_BITS."""
    return np.full(shape, NAN_BITS, np.int32).view(np.float32)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def equals_f64(got, ref):
    """float32 `got` equals the float64 `ref` exactly (as values: -0 == +0), and is finite."""
    got = np.asarray(got)
    return got.shape == ref.shape and bool(np.isfinite(got).all()) and np.array_equal(got.astype(F64), ref)


def worst_ratio(got, ref, bound):
    """max |got - ref| / bound; inf where got is not finite or where the bound is 0 and the error is not."""
    err = np.abs(np.asarray(got, F64) - ref)
    err = np.where(np.isfinite(err), err, np.inf)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / bound)
    return float(r.max()) if r.size else 0.0


# ---- Dormand-Prince 5(4): the stage rows and the error row b5 - b4 (csrc/step_ctl.h DP_A / DP_E) as the solver passes them, cast to float32 ----
DP_A = [[1 / 5], [3 / 40, 9 / 40], [44 / 45, -56 / 15, 32 / 9], [19372 / 6561, -25360 / 2187, 64448 / 6561, -212 / 729],
        [9017 / 3168, -355 / 33, 46732 / 5247, 49 / 176, -5103 / 18656], [35 / 384, 0.0, 500 / 1113, 125 / 192, -2187 / 6784, 11 / 84]]
DP_E = [35 / 384 - 5179 / 57600, 0.0, 500 / 1113 - 7571 / 16695, 125 / 192 - 393 / 640, -2187 / 6784 + 92097 / 339200, 11 / 84 - 187 / 2100,
        -1 / 40]


def dp_rows():
    """[(name, cx, coefficients as float32)]: the six stage rows (cx = 1) and the error row (cx = 0, 7 entries, one of them 0)."""
    rows = [(f"stage{i + 2}", 1.0, np.asarray(a, np.float32)) for i, a in enumerate(DP_A)]
    return rows + [("error", 0.0, np.asarray(DP_E, np.float32))]


# ---- ode_lincomb ------------------------------------------------------------------------------------------------------------------
LINCOMB_SIZES = (1, 255, 257, 768 * 64, 8192 * 256 + 257)     # the last: second trip of the grid-stride loop (8192 blocks x 256)
EXACT_COEFS = np.asarray([2, -1, 0.5, -0.25, 1, -2, 0.25], np.float32)


def kept_terms(ks, cs):
    """The terms the launcher keeps: k[j] given and c[j] != 0."""
    return [(k, np.float32(c)) for k, c in zip(ks, cs) if k is not None and c != 0]


def lincomb_ref(x, cx, dt, ks, cs):
    kept = kept_terms(ks, cs)
    s = np.zeros((kept[0][0] if kept else x).shape)
    for k, c in kept:
        s = s + F64(c) * k.astype(F64)
    out = F64(np.float32(dt)) * s
    return out + F64(np.float32(cx)) * x.astype(F64) if cx != 0 else out


def lincomb_bound(x, cx, dt, ks, cs):
    """(m + 3) u (|cx x| + |dt| sum |c_j k_j|), m = the terms kept.  The first term of the sum meets m roundings (its product or fma,
    then m - 1 sums), the scaling by dt one, the cx x fma one (two unfused: then |cx x| meets two): m + 2 at most, + 1 for the second order."""
    kept = kept_terms(ks, cs)
    mag = 0.0
    for k, c in kept:
        mag = mag + np.abs(F64(c) * k.astype(F64))
    mag = abs(F64(np.float32(dt))) * mag
    if cx != 0:
        mag = mag + np.abs(F64(np.float32(cx)) * x.astype(F64))
    return (len(kept) + 3) * U * mag


def lincomb_f32(x, cx, dt, ks, cs, fused):
    kept = kept_terms(ks, cs)
    s = np.zeros(kept[0][0].shape if kept else x.shape, np.float32)
    for k, c in kept:
        s = fma32(c, k, s, fused)
    o = mul32(np.float32(dt), s)
    return fma32(np.float32(cx), x, o, fused) if cx != 0 else o


def lincomb_exact_data(rng, n, nk):
    """Integers |x|, |k| <= 8 and coefficients in {+-2, +-1, +-1/2, +-1/4}: every partial sum is a multiple of 1/4 below 2^8, exact in float32
    fused or not; dt = 2^-3."""
    x = rng.integers(-8, 9, (n, 2)).astype(np.float32)
    ks = [rng.integers(-8, 9, (n, 2)).astype(np.float32) for _ in range(nk)]
    return x, ks, EXACT_COEFS[:nk], 0.125


def lincomb_random_data(rng, n, nk):
    return rng.standard_normal((n, 2)).astype(np.float32), [rng.standard_normal((n, 2)).astype(np.float32) for _ in range(nk)]


# ---- ode_scaled_sq ----------------------------------------------------------------------------------------------------------------
NORM_BLOCKS = 512                                               # DP_NORM_BLOCKS of csrc/solve.hip
NORM_SIZES = (1, 100, 768 * 64, 512 * 256 * 2 + 77)             # 768 * 64 < 512 * 256: blocks without an element
NORM_C = 20


def scaled_sq_terms(p, q, r, s, atol, rtol, r_only=False):
    d = p.astype(F64) - (0 if q is None else q.astype(F64))
    mr, ms = np.hypot(r[..., 0].astype(F64), r[..., 1].astype(F64)), np.hypot(s[..., 0].astype(F64), s[..., 1].astype(F64))
    sc = F64(np.float32(atol)) + F64(np.float32(rtol)) * (mr if r_only else np.maximum(mr, ms))
    return (d[..., 0] ** 2 + d[..., 1] ** 2) / sc ** 2


def scaled_sq_ref(p, q, r, s, atol, rtol, r_only=False):
    """sum |p - q|^2 / (atol + rtol max(|r|, |s|))^2 in float64 (r_only: the wrong norm that forgets s, for the tests' own check)."""
    return float(scaled_sq_terms(p, q, r, s, atol, rtol, r_only).sum())


def scaled_sq_block_ref(p, q, r, s, atol, rtol, nblocks=NORM_BLOCKS):
    """The float64 partial of every block: block j owns the elements i with (i // 256) % nblocks == j."""
    t = scaled_sq_terms(p, q, r, s, atol, rtol)
    owner = (np.arange(t.size) // 256) % nblocks
    return np.bincount(owner, weights=t, minlength=nblocks)


def scaled_sq_f32(p, q, r, s, atol, rtol, fused):
    """The kernel's term in float32, summed in float64."""
    d = p if q is None else add32(p, -q)
    sq = lambda v: fma32(v[..., 0], v[..., 0], mul32(v[..., 1], v[..., 1]), fused)
    m = np.maximum(np.sqrt(sq(r)), np.sqrt(sq(s)))               # np.sqrt and / on float32 are correctly rounded, as sqrtf and / are without fast-math
    sc = fma32(np.float32(rtol), m, np.float32(atol), fused)
    return float((sq(d) / mul32(sc, sc)).astype(F64).sum())


def scaled_sq_data(rng, n, exact):
    """p, q, r, s.  exact: integer p, q with |p - q| <= 16 (used with atol = 2^-3, rtol = 0: every term is an integer times 64)."""
    if exact:
        p, q = (rng.integers(-8, 9, (n, 2)).astype(np.float32) for _ in range(2))
    else:
        p, q = (rng.standard_normal((n, 2)).astype(np.float32) for _ in range(2))
    r, s = (rng.standard_normal((n, 2)).astype(np.float32) for _ in range(2))
    if n >= 2:                                                    # each side wins the max somewhere, whatever the draw
        r[0], s[0] = (3.0, 4.0), (0.5, 0.0)
        r[1], s[1] = (0.0, 0.5), (-4.0, 3.0)
    return p, q, r, s


# ---- output layer + updates -------------------------------------------------------------------------------------------------------
IMAGE_SHAPES = ((3, 5, 7), (2, 1, 9), (2, 8, 1), (1, 768, 4))


def output_layer_ref(pyr, w, absolute=False):
    """The output layer (4 -> 2, no bias; w [2][4] or [2][4][3][3], zero padding 'same' per image) of pyr [B][H][W][4] in float64 ->
    [B][H][W][2]; absolute: the sum of the magnitudes of the products instead."""
    p, w = pyr.astype(F64), np.asarray(w, F64)
    f = np.abs if absolute else (lambda a: a)
    if w.ndim == 2:
        return np.einsum("bhwc,oc->bhwo", f(p), f(w))
    B, H, W, _ = p.shape
    pp = np.zeros((B, H + 2, W + 2, 4))
    pp[:, 1:-1, 1:-1] = f(p)
    out = np.zeros((B, H, W, 2))
    for dy in range(3):
        for dx in range(3):
            out += np.einsum("bhwc,oc->bhwo", pp[:, dy:dy + H, dx:dx + W], f(w[:, :, dy, dx]))
    return out


def output_layer_f32(pyr, w, fused):
    w = np.asarray(w, np.float32)
    B, H, W, _ = pyr.shape
    if w.ndim == 2:
        cols = []
        for o in range(2):
            acc = mul32(w[o, 0], pyr[..., 0])
            for ci in range(1, 4):
                acc = fma32(w[o, ci], pyr[..., ci], acc, fused)
            cols.append(acc)
        return np.stack(cols, -1)
    # taps ascending, channels ascending per tap, from 0; a tap outside the image is skipped (adding its exact zero product changes nothing)
    pp = np.zeros((B, H + 2, W + 2, 4), np.float32)
    pp[:, 1:-1, 1:-1] = pyr
    cols = []
    for o in range(2):
        acc = np.zeros((B, H, W), np.float32)
        for dy in range(3):
            for dx in range(3):
                for ci in range(4):
                    acc = fma32(w[o, ci, dy, dx], pp[:, dy:dy + H, dx:dx + W, ci], acc, fused)
        cols.append(acc)
    return np.stack(cols, -1)


def taps(w):
    return 4 if np.ndim(w) == 2 else 36


def output_update_ref(pyr, w, base, kold, coef):
    """-> (dst, ksave) in float64: ksave = v, dst = base + coef (v + kold); base / kold None = absent."""
    v = output_layer_ref(pyr, w)
    s = v if kold is None else v + kold.astype(F64)
    o = F64(np.float32(coef)) * s
    return (o if base is None else o + base.astype(F64)), v


def output_update_bound(pyr, w, base, kold, coef):
    """(t + 3) u (sum of magnitudes), t = 4 or 36 taps: a product of v meets at most t roundings in the layer (its own, then the sums after
    it), then + kold, * coef, + base: t + 3.  -> (bound of dst, bound of ksave: the same count on v's own magnitudes)."""
    va = output_layer_ref(pyr, w, absolute=True)
    mag = abs(F64(np.float32(coef))) * (va + (0 if kold is None else np.abs(kold.astype(F64)))) + (0 if base is None else np.abs(base.astype(F64)))
    return (taps(w) + 3) * U * mag, (taps(w) + 3) * U * va


def output_update_f32(pyr, w, base, kold, coef, fused):
    v = output_layer_f32(pyr, w, fused)
    s = v if kold is None else add32(v, kold)
    o = mul32(np.float32(coef), s)
    return (o if base is None else add32(o, base)), v


def score_update_ref(pyr, w, base, cb, Y, cy, cn, z, cz):
    c = lambda v: F64(np.float32(v))
    o = c(cb) * base.astype(F64) + c(cn) * output_layer_ref(pyr, w)
    if cy != 0:
        o = o + c(cy) * Y.astype(F64)
    if cz != 0:
        o = o + c(cz) * z.astype(F64)
    return o


def score_update_bound(pyr, w, base, cb, Y, cy, cn, z, cz):
    """(t + 3) u (|cb base| + |cy Y| + |cn| sum |w p| + |cz z|): a product of v meets t roundings in the layer and one in each of the three
    fmas after it; cb base its own and the same three."""
    c = lambda v: abs(F64(np.float32(v)))
    mag = c(cb) * np.abs(base.astype(F64)) + c(cn) * output_layer_ref(pyr, w, absolute=True)
    if cy != 0:
        mag = mag + c(cy) * np.abs(Y.astype(F64))
    if cz != 0:
        mag = mag + c(cz) * np.abs(z.astype(F64))
    return (taps(w) + 3) * U * mag


def score_update_f32(pyr, w, base, cb, Y, cy, cn, z, cz, fused):
    o = fma32(np.float32(cn), output_layer_f32(pyr, w, fused), mul32(np.float32(cb), base), fused)
    if cy != 0:
        o = fma32(np.float32(cy), Y, o, fused)
    if cz != 0:
        o = fma32(np.float32(cz), z, o, fused)
    return o


def output_weights(rng, ks, exact):
    """[2][4] or [2][4][3][3] float32; exact: multiples of 1/4 in [-2, 2]."""
    shape = (2, 4) if ks == 1 else (2, 4, 3, 3)
    if exact:
        return (rng.integers(-8, 9, shape) / 4).astype(np.float32)
    return (rng.standard_normal(shape) / np.sqrt(4 * ks * ks)).astype(np.float32)


def image_data(rng, shape, dtype, exact):
    """pyr [B][H][W][4] as stored in `dtype`, and four complex planes [B][H][W][2] (base, kold / Y, z, spare).  exact: integers, |pyr| <= 4
    (exact in bf16), planes |.| <= 8: with the weights above |v| <= 288 in steps of 1/4 and every later sum stays far below 2^24 of them.
    Every image and every row differs from the others (random data): a read across a boundary changes the result."""
    B, H, W = shape
    if exact:
        pyr = rng.integers(-4, 5, (B, H, W, 4)).astype(np.float32)
        planes = [rng.integers(-8, 9, (B, H, W, 2)).astype(np.float32) for _ in range(4)]
    else:
        pyr = stored(rng.standard_normal((B, H, W, 4)).astype(np.float32), dtype)
        planes = [rng.standard_normal((B, H, W, 2)).astype(np.float32) for _ in range(4)]
    return pyr, planes


def regions(H, W):
    """Named index sets of an H x W image: the four borders, the corners and the interior, as boolean masks [H][W]."""
    hh, ww = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    top, bottom, left, right = hh == 0, hh == H - 1, ww == 0, ww == W - 1
    return {"top": top, "bottom": bottom, "left": left, "right": right, "corners": (top | bottom) & (left | right),
            "interior": ~(top | bottom | left | right)}


# ---- init_state and caxpy -----------------------------------------------------------------------------------------------------------
def sigma_curve(F, exact):
    """float64 [F], varying strongly with f: 2^(f mod 7) (1 + f / 8) -- dyadic, so that with integer noise sigma z is exact in float32."""
    f = np.arange(F, dtype=F64)
    s = 2.0 ** (f % 7) * (1 + f / 8)
    return s if exact else s * (1 + 1e-3 * np.sin(f))           # not representable in float32: the float64 product matters


def scaled_noise(sigma, z):
    """nx = float32(sigma[f] * float64(z)), exactly as the kernel forms it; sigma [1] or [F], z [B][F][T][2]."""
    s = np.asarray(sigma, F64)
    s = s[0] if s.size == 1 else s[None, :, None, None]
    return f32(s * z.astype(F64))


def init_state_ref(Y, sigma, sigma_fac, z):
    return Y.astype(F64) + F64(np.float32(sigma_fac)) * scaled_noise(sigma, z).astype(F64)


def init_state_bound(Y, sigma, sigma_fac, z):
    """2 u (|Y| + |sigma_fac nx|): the product and the sum, or one fma."""
    return 2 * U * (np.abs(Y.astype(F64)) + np.abs(F64(np.float32(sigma_fac)) * scaled_noise(sigma, z).astype(F64)))


def init_state_f32(Y, sigma, sigma_fac, z, fused):
    return fma32(np.float32(sigma_fac), scaled_noise(sigma, z), Y, fused)


def caxpy_ref(a, cq, q):
    return a.astype(F64) + F64(np.float32(cq)) * q.astype(F64)


def caxpy_bound(a, cq, q):
    """2 u (|a| + |cq q|): one fma, or a product and a sum."""
    return 2 * U * (np.abs(a.astype(F64)) + np.abs(F64(np.float32(cq)) * q.astype(F64)))


def caxpy_f32(a, cq, q, fused):
    return fma32(np.float32(cq), q, a, fused)


def plane_data(rng, shape, exact):
    """Two complex planes [B][F][T][2]; exact: integers |.| <= 8."""
    if exact:
        return [rng.integers(-8, 9, shape + (2,)).astype(np.float32) for _ in range(2)]
    return [rng.standard_normal(shape + (2,)).astype(np.float32) for _ in range(2)]


# ---- pack_input and combine -------------------------------------------------------------------------------------------------------
COMBINE_COUTS = (8, 64, 256)                                     # 1, 8 and 32 threads per pixel
COMBINE_HW = ((16, 16), (1, 257), (20, 30), (1, 64 * 3 + 5))     # HW = 256, 257, 600, 197: whole tile, one pixel over, ragged, short
COMBINE_PX = 256


def pack_ref(x, y, dtype):
    """-> [..., 8] float32: (x.re, x.im, y.re, y.im) as stored in dtype, then four zeros."""
    out = np.zeros(x.shape[:-1] + (8,), np.float32)
    out[..., 0:2], out[..., 2:4] = stored(x, dtype), stored(y, dtype)
    return out


def combine_ref(p4, w, bias, h):
    """conv1x1(p4[..., :4]) + bias + h in float64; p4 [B][H][W][8], w [Cout][4], h [B][H][W][Cout]."""
    return np.einsum("bhwc,oc->bhwo", p4[..., :4].astype(F64), w.astype(F64)) + bias.astype(F64) + h.astype(F64)


def combine_bound(p4, w, bias, h, dtype):
    """Of the STORED value: the float32 result is within 6 u mag of the reference, mag = |bias| + sum |w p| + |h| (the bias meets the four
    fmas and the sum with h: 5 roundings, + 1 for the second order); storing as bf16 adds 2^-8 of that result's magnitude."""
    mag = np.einsum("bhwc,oc->bhwo", np.abs(p4[..., :4].astype(F64)), np.abs(w.astype(F64))) + np.abs(bias.astype(F64)) + np.abs(h.astype(F64))
    e32 = 6 * U * mag
    return e32 if dtype == "fp32" else e32 + U_BF16 * (np.abs(combine_ref(p4, w, bias, h)) + e32)


def combine_f32(p4, w, bias, h, dtype, fused):
    B, H, W, _ = p4.shape
    acc = np.broadcast_to(bias.astype(np.float32), (B, H, W, w.shape[0])).copy()
    for ci in range(4):
        acc = fma32(w[None, None, None, :, ci], p4[..., ci:ci + 1], acc, fused)
    return stored(add32(acc, h), dtype)


def tile_sums(out):
    """(sum, sum of squares, sum of magnitudes) per 256-pixel tile and channel of out [B][H][W][C], in float64 -> three [B][tiles][C]."""
    B, H, W, C = out.shape
    HW = H * W
    tiles = -(-HW // COMBINE_PX)
    o = np.zeros((B, tiles * COMBINE_PX, C))
    o[:, :HW] = out.reshape(B, HW, C).astype(F64)
    o = o.reshape(B, tiles, COMBINE_PX, C)
    return o.sum(2), (o * o).sum(2), np.abs(o).sum(2)


def stats_bound(out):
    """256 u relative per partial: a float32 sum of at most 256 values -- 256 u sum |q| for the sum, 256 u sum q^2 for the squares (their
    products are fused into the sum or add one rounding to a chain that is at most 255 long)."""
    _, ss, sa = tile_sums(out)
    return COMBINE_PX * U * sa, COMBINE_PX * U * ss


def stats_f32(out, fused):
    """Float32 sums in pixel order (one possible order of the kernel's; the bound does not depend on the order)."""
    B, H, W, C = out.shape
    HW = H * W
    tiles = -(-HW // COMBINE_PX)
    q = out.reshape(B, HW, C).astype(np.float32)
    s, ss = np.zeros((B, tiles, C), np.float32), np.zeros((B, tiles, C), np.float32)
    for p in range(HW):
        t = p // COMBINE_PX
        s[:, t] = add32(s[:, t], q[:, p])
        ss[:, t] = fma32(q[:, p], q[:, p], ss[:, t], fused)
    return s, ss


def combine_data(rng, B, H, W, Cout, dtype, exact):
    """p4 [B][H][W][8] (channels 4..7 hold NaN: the kernel must not read them), w, bias, h.  exact: integers |p4|, |h| <= 3 and w, bias in
    {0, +-1}: |out| <= 4 * 3 + 1 + 3 = 16, exact in bf16, and a tile's sums stay below 256 * 16^2 = 2^16."""
    p4 = sentinel((B, H, W, 8)).copy()
    if exact:
        p4[..., :4] = rng.integers(-3, 4, (B, H, W, 4))
        w, bias = rng.integers(-1, 2, (Cout, 4)).astype(np.float32), rng.integers(-1, 2, Cout).astype(np.float32)
        h = rng.integers(-3, 4, (B, H, W, Cout)).astype(np.float32)
    else:
        p4[..., :4] = stored(rng.standard_normal((B, H, W, 4)).astype(np.float32), dtype)
        w, bias = (0.5 * rng.standard_normal((Cout, 4))).astype(np.float32), rng.standard_normal(Cout).astype(np.float32)
        h = stored(rng.standard_normal((B, H, W, Cout)).astype(np.float32), dtype)
    return p4, w, bias, h


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def refusal_cases(lib, p, dt):
    """[(label, call, message)]: one call per argument check of every wrapper; `p` = any valid non-null pointer (never dereferenced: a refused
    call launches nothing), dt = a dtype id.  Shared with the GPU test, which passes device buffers and checks that they stay untouched."""
    kp, cp = (C.c_void_p * 8)(*([p.value] * 8)), (C.c_float * 8)(*([1.0] * 8))
    N = None
    return [
        ("pack null", lambda: lib.fd_op_pack_input(p, N, p, 1, 4, 4, dt, N), "null pointer"),
        ("pack dtype", lambda: lib.fd_op_pack_input(p, p, p, 1, 4, 4, 7, N), "dtype"),
        ("pack shape", lambda: lib.fd_op_pack_input(p, p, p, 0, 4, 4, dt, N), "bad shape"),
        ("combine null", lambda: lib.fd_op_combine(p, p, p, p, p, N, 1, 4, 4, 8, dt, N), "null pointer"),
        ("combine B", lambda: lib.fd_op_combine(p, p, p, p, p, p, 65536, 4, 4, 8, dt, N), "65535"),
        ("combine B0", lambda: lib.fd_op_combine(p, p, p, p, p, p, 0, 4, 4, 8, dt, N), "bad shape"),
        ("combine Cout 24", lambda: lib.fd_op_combine(p, p, p, p, p, p, 1, 4, 4, 24, dt, N), "power of two"),
        ("combine Cout 4", lambda: lib.fd_op_combine(p, p, p, p, p, p, 1, 4, 4, 4, dt, N), "power of two"),
        ("combine Cout 512", lambda: lib.fd_op_combine(p, p, p, p, p, p, 1, 4, 4, 512, dt, N), "power of two"),
        ("output null", lambda: lib.fd_op_output_update(p, p, p, p, 1.0, N, p, 1, 4, 4, 1, dt, N), "null pointer"),
        ("output ks", lambda: lib.fd_op_output_update(p, p, p, p, 1.0, p, p, 1, 4, 4, 2, dt, N), "ks must be 1 or 3"),
        ("output dtype", lambda: lib.fd_op_output_update(p, p, p, p, 1.0, p, p, 1, 4, 4, 1, -1, N), "dtype"),
        ("score null base", lambda: lib.fd_op_score_update(p, p, N, 1.0, p, 1.0, 1.0, p, N, 0, 1.0, p, 1, 4, 4, 1, dt, N), "null pointer"),
        ("score null Y", lambda: lib.fd_op_score_update(p, p, p, 1.0, N, 1.0, 1.0, p, N, 0, 1.0, p, 1, 4, 4, 1, dt, N), "Y with cy"),
        ("score ks", lambda: lib.fd_op_score_update(p, p, p, 1.0, p, 1.0, 1.0, p, N, 0, 1.0, p, 1, 4, 4, 5, dt, N), "ks must be 1 or 3"),
        ("score both", lambda: lib.fd_op_score_update(p, p, p, 1.0, p, 1.0, 1.0, p, p, 0, 1.0, p, 1, 4, 4, 1, dt, N), "exactly one"),
        ("score neither", lambda: lib.fd_op_score_update(p, p, p, 1.0, p, 1.0, 1.0, N, N, 0, 1.0, p, 1, 4, 4, 1, dt, N), "exactly one"),
        ("score both cz 0", lambda: lib.fd_op_score_update(p, p, p, 1.0, p, 1.0, 1.0, p, p, 0, 0.0, p, 1, 4, 4, 1, dt, N), "exactly one"),
        ("init null", lambda: lib.fd_op_init_state(p, p, N, N, 0, N, 1, 1.0, p, 1, 4, 4, N), "null pointer"),
        ("init both", lambda: lib.fd_op_init_state(p, p, p, N, 0, p, 1, 1.0, p, 1, 4, 4, N), "exactly one"),
        ("init neither", lambda: lib.fd_op_init_state(p, N, N, N, 0, p, 1, 1.0, p, 1, 4, 4, N), "exactly one"),
        ("init sigma_n", lambda: lib.fd_op_init_state(p, p, N, N, 0, p, 3, 1.0, p, 1, 4, 4, N), "sigma_n"),
        ("init frame0", lambda: lib.fd_op_init_state(p, p, N, p, 0, p, 1, 1.0, p, 1, 4, 4, N), "frame0 needs seeds"),
        ("init draw", lambda: lib.fd_op_init_state(p, N, p, N, -1, p, 1, 1.0, p, 1, 4, 4, N), "draw"),
        ("caxpy null", lambda: lib.fd_op_caxpy(N, p, N, 0, 1.0, p, 1, 4, 4, N), "null pointer"),
        ("caxpy both", lambda: lib.fd_op_caxpy(p, p, p, 0, 1.0, p, 1, 4, 4, N), "exactly one"),
        ("caxpy neither", lambda: lib.fd_op_caxpy(p, N, N, 0, 1.0, p, 1, 4, 4, N), "exactly one"),
        ("caxpy shape", lambda: lib.fd_op_caxpy(p, p, N, 0, 1.0, p, 1, 0, 4, N), "bad shape"),
        ("lincomb nk", lambda: lib.fd_op_ode_lincomb(p, 1.0, 1.0, kp, cp, 8, p, 16, N), "nk must be in [0, 7]"),
        ("lincomb dst", lambda: lib.fd_op_ode_lincomb(p, 1.0, 1.0, kp, cp, 1, N, 16, N), "null pointer"),
        ("lincomb x", lambda: lib.fd_op_ode_lincomb(N, 1.0, 1.0, kp, cp, 1, p, 16, N), "null pointer"),
        ("lincomb tables", lambda: lib.fd_op_ode_lincomb(p, 1.0, 1.0, None, cp, 1, p, 16, N), "null pointer"),
        ("lincomb n", lambda: lib.fd_op_ode_lincomb(p, 1.0, 1.0, kp, cp, 1, p, 0, N), "element count"),
        ("lincomb_clips nk", lambda: lib.fd_op_ode_lincomb_clips(p, 1.0, p, kp, cp, 8, p, 1, 16, N), "nk must be in [0, 7]"),
        ("lincomb_clips dt", lambda: lib.fd_op_ode_lincomb_clips(p, 1.0, N, kp, cp, 1, p, 1, 16, N), "null pointer"),
        ("lincomb_clips B 0", lambda: lib.fd_op_ode_lincomb_clips(p, 1.0, p, kp, cp, 1, p, 0, 16, N), "65535"),
        ("lincomb_clips B", lambda: lib.fd_op_ode_lincomb_clips(p, 1.0, p, kp, cp, 1, p, 65536, 16, N), "65535"),
        ("scaled_sq null", lambda: lib.fd_op_ode_scaled_sq(p, p, p, p, 1.0, 1.0, N, 512, 16, N), "null pointer"),
        ("scaled_sq nblocks", lambda: lib.fd_op_ode_scaled_sq(p, p, p, p, 1.0, 1.0, p, 0, 16, N), "nblocks"),
        ("scaled_sq_clips nblocks", lambda: lib.fd_op_ode_scaled_sq_clips(p, p, p, p, 1.0, 1.0, p, 0, 1, 16, N), "nblocks"),
        ("scaled_sq_clips B", lambda: lib.fd_op_ode_scaled_sq_clips(p, p, p, p, 1.0, 1.0, p, 512, 65536, 16, N), "65535"),
        ("scaled_sq_clips null", lambda: lib.fd_op_ode_scaled_sq_clips(p, p, N, p, 1.0, 1.0, p, 512, 1, 16, N), "null pointer"),
        ("commit null", lambda: lib.fd_op_ode_commit_clips(p, N, p, p, p, p, p, 1, 16, N), "null pointer"),
        ("commit B 0", lambda: lib.fd_op_ode_commit_clips(p, p, p, p, p, p, p, 0, 16, N), "65535"),
        ("commit B", lambda: lib.fd_op_ode_commit_clips(p, p, p, p, p, p, p, 65536, 16, N), "65535"),
        ("commit n", lambda: lib.fd_op_ode_commit_clips(p, p, p, p, p, p, N, 1, 0, N), "element count"),
    ]
