"""The kernels between the network and the ODE / SDE solvers, one at a time, on the GPU (include/flowdec_hip.h "Operator-level: solver and
edge kernels"; csrc/net_edges.hip and csrc/solver_ops.hip through csrc/ops_api.hip, whose wrappers call the launchers the model and the solvers call).

Every reference is NumPy float64 computed from the stored inputs, every bound is derived from the kernel's operation count
(tests/solver_ops_ref.py; tests/test_solver_ops_cpu.py shows that the float32 arithmetic itself meets them, fused or not), every output is
prefilled with NaNs so that an unwritten element fails, and 'exact' data sets make every intermediate representable: there the result
equals float64 bit for bit.  The one measured number per test, the worst error / bound, goes to the parity report."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import solver_ops_ref as R
from test_hip_ops import REPORT     # the parity report every GPU test module appends to

pytestmark = pytest.mark.gpu

DT = {"bf16": torch.bfloat16, "fp32": torch.float32}
BIG = R.LINCOMB_SIZES[-1]


class Check:
    """Collects the checks of one test: the worst error / bound, and every failure; done() writes the report line, then asserts."""

    def __init__(self, name):
        self.name, self.ratio, self.fails = name, 0.0, []

    def bounded(self, what, got, ref, bound):
        r = R.worst_ratio(got, ref, bound)
        self.ratio = max(self.ratio, r)
        if not r <= 1.0:
            self.fails.append(f"{what}: error / bound = {r:.3f}")

    def true(self, what, ok):
        if not ok:
            self.ratio = float("inf")
            self.fails.append(what)

    def exact(self, what, got, ref):
        self.true(f"{what}: differs from float64", R.equals_f64(got, ref))

    def image(self, what, got, ref, bound=None):
        """[B][H][W][2] results, asserted separately on the four borders, the corners and the interior (bound None: exact)."""
        for region, mask in R.regions(*got.shape[1:3]).items():
            if mask.any():
                g, r = got[:, mask], ref[:, mask]
                self.exact(f"{what} {region}", g, r) if bound is None else self.bounded(f"{what} {region}", g, r, bound[:, mask])

    def done(self):
        os.makedirs(os.path.dirname(REPORT), exist_ok=True)
        with open(REPORT, "a") as f:
            f.write(f"{self.name:60s} err/bound={self.ratio:.3e} {'OK' if not self.fails else 'FAIL'}\n")
        print(f"{self.name}: worst error / bound = {self.ratio:.3e}")
        assert not self.fails, f"{len(self.fails)} checks failed: " + "; ".join(self.fails[:6])


@pytest.fixture
def chk(request):
    return Check("solver_ops." + request.node.name.replace("test_", "", 1))


@pytest.fixture(scope="module")
def ops():
    from flowdec_amd import ops as _ops
    return _ops


def plane(a):
    """float32 [..., 2] -> complex64 tensor on the GPU (the same bits)."""
    return torch.view_as_complex(torch.from_numpy(np.ascontiguousarray(a, np.float32))).cuda()


def nans(*shape):
    """A complex64 output prefilled with the sentinel NaN."""
    return plane(R.sentinel(tuple(shape) + (2,)))


def back(t):
    return torch.view_as_real(t).cpu().numpy()


def nhwc(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda().to(DT[dtype])


def seeds_of(*vals):
    from flowdec_amd.noise import seeds_to_tensor
    return seeds_to_tensor(list(vals), len(vals), "cuda")


# ---- ode_lincomb / ode_lincomb_clips --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", R.LINCOMB_SIZES)
def test_lincomb_exact(ops, chk, n):
    rng = np.random.default_rng(n)
    for nk in (1, 6, 7):
        x, ks, cs, dt = R.lincomb_exact_data(rng, n, nk)
        dx, dks = plane(x), [plane(k) for k in ks]
        for cx in ((1.0, -0.5, 0.0) if n < BIG or nk == 7 else (1.0,)):
            got = back(ops.ode_lincomb(dx, cx, dt, dks, cs, nans(n)))
            chk.exact(f"nk={nk} cx={cx}", got, R.lincomb_ref(x, cx, dt, ks, cs))
    chk.done()


@pytest.mark.parametrize("n", R.LINCOMB_SIZES)
def test_lincomb_dopri_rows(ops, chk, n):
    """|got - ref| <= (m + 3) u (|cx x| + |dt| sum |c_j k_j|) per component (solver_ops_ref.lincomb_bound), on the float32 Dormand-Prince rows."""
    rng = np.random.default_rng(n + 1)
    x, ks = R.lincomb_random_data(rng, n, 7)
    dx, dks = plane(x), [plane(k) for k in ks]
    for name, cx, cs in (R.dp_rows() if n < BIG else R.dp_rows()[-2:]):
        nk, dt = len(cs), 0.0371
        got = back(ops.ode_lincomb(dx, cx, dt, dks[:nk], cs, nans(n)))
        chk.bounded(name, got, R.lincomb_ref(x, cx, dt, ks[:nk], cs), R.lincomb_bound(x, cx, dt, ks[:nk], cs))
    chk.done()


def test_lincomb_contracts(ops, chk):
    """cx = 0: x is not read; c_j = 0 or a null k_j: the term is skipped; dt = 0 with cx = 1 returns x bit for bit."""
    n = 257
    rng = np.random.default_rng(7)
    x, ks = R.lincomb_random_data(rng, n, 3)
    dx, dks, bad = plane(x), [plane(k) for k in ks], nans(n)
    cs = np.asarray([0.3, -1.7, 0.9], np.float32)
    ref0 = R.lincomb_ref(x, 0.0, 0.5, ks, cs)
    bound0 = R.lincomb_bound(x, 0.0, 0.5, ks, cs)
    chk.bounded("cx = 0, NaNs in x", back(ops.ode_lincomb(bad, 0.0, 0.5, dks, cs, nans(n))), ref0, bound0)
    chk.bounded("cx = 0, x null", back(ops.ode_lincomb(None, 0.0, 0.5, dks, cs, nans(n))), ref0, bound0)
    cz = np.asarray([0.3, 0.0, 0.9], np.float32)
    ref1, bound1 = R.lincomb_ref(x, 1.0, 0.5, ks, cz), R.lincomb_bound(x, 1.0, 0.5, ks, cz)
    got = back(ops.ode_lincomb(dx, 1.0, 0.5, [dks[0], bad, dks[2]], cz, nans(n)))
    chk.bounded("c_1 = 0, NaNs in k_1", got, ref1, bound1)
    chk.true("a null k_1 gives other bits than c_1 = 0", R.same_bits(back(ops.ode_lincomb(dx, 1.0, 0.5, [dks[0], None, dks[2]], cs, nans(n))), got))
    chk.true("dt = 0, cx = 1 does not return x", R.same_bits(back(ops.ode_lincomb(dx, 1.0, 0.0, dks, cs, nans(n))), x))
    chk.true("nk = 0, cx = 1 does not return x", R.same_bits(back(ops.ode_lincomb(dx, 1.0, 0.5, [], [], nans(n))), x))
    chk.done()


@pytest.mark.parametrize("B,n,row", [(1, 257, 6), (3, 768 * 64, 6), (3, 768 * 64, 5), (256, 257, 5), (3, BIG, 1)],
                         ids=["B1", "B3_error_row", "B3_stage7", "B256", "B3_second_trip"])
def test_lincomb_clips(ops, chk, B, n, row):
    """Per-clip steps dt[b] (some of them 0): clip b == the batch-global launch on clip b alone, bit for bit, and within the bound of float64."""
    rng = np.random.default_rng(B * 1000 + row)
    name, cx, cs = R.dp_rows()[row]
    nk = len(cs)
    x, ks = R.lincomb_random_data(rng, B * n, nk)
    x, ks = x.reshape(B, n, 2), [k.reshape(B, n, 2) for k in ks]
    dt = np.asarray([0.0 if b % 3 == 1 else 0.0371 / (b + 1) for b in range(B)], np.float32)
    dx, dks, ddt = plane(x), [plane(k) for k in ks], torch.from_numpy(dt).cuda()
    got_t = ops.ode_lincomb(dx, cx, ddt, dks, cs, nans(B, n))
    got = back(got_t)
    for b in range(B):
        single = ops.ode_lincomb(dx[b], cx, float(dt[b]), [k[b] for k in dks], cs, nans(n))
        chk.true(f"clip {b} differs from the launch on the clip alone", bool(torch.equal(torch.view_as_real(single).view(torch.int32),
                                                                                        torch.view_as_real(got_t[b]).view(torch.int32))))
        if b < 4 or b == B - 1:
            kb = [k[b] for k in ks]
            chk.bounded(f"{name} clip {b}", got[b], R.lincomb_ref(x[b], cx, dt[b], kb, cs), R.lincomb_bound(x[b], cx, dt[b], kb, cs))
        if dt[b] == 0 and cx == 1.0:
            chk.true(f"finished clip {b} (dt = 0) is not x", R.same_bits(got[b], x[b]))
    chk.done()


# ---- ode_scaled_sq / ode_scaled_sq_clips ------------------------------------------------------------------------------------------------
def partials(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float64, device="cuda")


@pytest.mark.parametrize("with_q", [True, False], ids=["q", "q_null"])
@pytest.mark.parametrize("n", R.NORM_SIZES)
def test_scaled_sq_exact(ops, chk, n, with_q):
    """atol = 2^-3, rtol = 0, integer p and q: every term is an integer times 64, so every block's partial -- 0.0 for a block that owns no
    element -- and their sum equal float64 exactly."""
    p, q, r, s = R.scaled_sq_data(np.random.default_rng(n), n, exact=True)
    q = q if with_q else None
    got = ops.ode_scaled_sq(plane(p), None if q is None else plane(q), plane(r), plane(s), 0.125, 0.0, out=partials(R.NORM_BLOCKS)).cpu().numpy()
    ref = R.scaled_sq_block_ref(p, q, r, s, 0.125, 0.0)
    chk.true("a block's partial differs from float64", np.array_equal(got, ref))
    chk.true("the sum of the partials differs from float64", float(got.sum()) == R.scaled_sq_ref(p, q, r, s, 0.125, 0.0))
    chk.true("a block without elements does not hold 0.0", not got[-(-n // 256):].any() and not np.isnan(got).any())
    chk.done()


@pytest.mark.parametrize("with_q", [True, False], ids=["q", "q_null"])
@pytest.mark.parametrize("n", R.NORM_SIZES)
def test_scaled_sq_random(ops, chk, n, with_q):
    """|sum(partials) - ref| <= c u ref with c = 20.  Roundings a term meets, in units of u, to first order: p - q 1 per component, so 2 on
    |d|^2; the two squares and their sum 1 + 1 -> 4 on the numerator.  Each modulus: square 1, sum 1, halved by the square root, + 1 for the
    root itself -> 2; the maximum is exact; rtol * m 1 -> 3; atol + . 1 -> 4 (both terms positive); squared 2 * 4 + 1 -> 9.  The quotient
    4 + 9 + 1 = 14.  The float64 accumulation adds n 2^-53 << u; c = 20 leaves the rest to the second order.  Division and square root are
    correctly rounded (no fast-math), a contracted multiply-add only removes a rounding."""
    p, q, r, s = R.scaled_sq_data(np.random.default_rng(n + 1), n, exact=False)
    q = q if with_q else None
    mr, ms = np.hypot(r[:, 0], r[:, 1]), np.hypot(s[:, 0], s[:, 1])
    for atol, rtol in ((1e-5, 1e-5), (1e-3, 0.05)):
        got = ops.ode_scaled_sq(plane(p), None if q is None else plane(q), plane(r), plane(s), atol, rtol, out=partials(R.NORM_BLOCKS)).cpu().numpy()
        ref = R.scaled_sq_ref(p, q, r, s, atol, rtol)
        chk.bounded(f"atol={atol} rtol={rtol}", np.asarray([got.sum()]), np.asarray([ref]), np.asarray([R.NORM_C * R.U * ref]))
        if n >= 2:   # each side wins the max somewhere, and the norm that forgets s would be caught
            chk.true("the data do not tell max(|r|, |s|) from |r|", bool((mr > ms).any() and (ms > mr).any())
                     and abs(R.scaled_sq_ref(p, q, r, s, atol, rtol, r_only=True) - ref) > 100 * R.NORM_C * R.U * ref)
    chk.done()


@pytest.mark.parametrize("with_q", [True, False], ids=["q", "q_null"])
def test_scaled_sq_clips(ops, chk, with_q):
    """partial[b][j] == partial[j] of the one-clip launch on clip b, bit for bit (B = 3), and every clip's sum is within the bound."""
    B = 3
    for n in (100, 768 * 64):
        p, q, r, s = (a.reshape(B, n, 2) for a in R.scaled_sq_data(np.random.default_rng(n + 2), B * n, exact=False))
        q = q if with_q else None
        dp, dq, dr, ds = plane(p), None if q is None else plane(q), plane(r), plane(s)
        got = ops.ode_scaled_sq(dp, dq, dr, ds, 1e-3, 0.05, clips=B, out=partials(B, R.NORM_BLOCKS)).cpu().numpy()
        for b in range(B):
            one = ops.ode_scaled_sq(dp[b], None if q is None else dq[b], dr[b], ds[b], 1e-3, 0.05, out=partials(R.NORM_BLOCKS)).cpu().numpy()
            chk.true(f"n={n} clip {b}: partials differ from the one-clip launch", np.array_equal(one.view(np.int64), got[b].view(np.int64)))
            ref = R.scaled_sq_ref(p[b], None if q is None else q[b], r[b], s[b], 1e-3, 0.05)
            chk.bounded(f"n={n} clip {b}", np.asarray([got[b].sum()]), np.asarray([ref]), np.asarray([R.NORM_C * R.U * ref]))
    chk.done()


# ---- ode_commit_clips ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [257, 8192 * 256 + 1])
@pytest.mark.parametrize("B", [1, 5])
def test_commit_clips(ops, chk, B, n):
    """Exact copies under mixed accept / ckpt in {0, 1, N}; rejected clips' x and k0 and every traj plane not addressed keep their sentinel."""
    N = 2
    m = B * n * 2
    # every element its own bit pattern (small integers as float bits: copied, never computed with)
    x_new = np.arange(m, dtype=np.int32).reshape(B, n, 2)
    k6 = x_new + (1 << 30)
    accepts = ([1], [0]) if B == 1 else ([1, 0, 1, 1, 0], [0, 0, 0, 0, 0])
    ckpts = ([N], [1]) if B == 1 else ([0, 1, N, 1, N], [1, 1, 1, 1, 1])
    # the bit patterns live on the GPU as int32 and are compared there (the trajectory of the large case is 250 MB)
    as_plane = lambda t: torch.view_as_complex(t.view(torch.float32))
    as_bits = lambda t: torch.view_as_real(t).view(torch.int32)
    filled = lambda *shape: torch.full(shape + (2,), R.NAN_BITS, dtype=torch.int32, device="cuda")
    same = lambda a, b: bool(torch.equal(a, b))
    untouched = lambda a: bool((a == R.NAN_BITS).all())
    bx, bk = torch.from_numpy(x_new).cuda(), torch.from_numpy(k6).cuda()
    for accept, ckpt in zip(accepts, ckpts):
        for with_traj in (True, False):
            if n > 257 and not any(accept):
                continue                                          # (the all-rejected launch is covered at n = 257)
            x, k0 = as_plane(filled(B, n)), as_plane(filled(B, n))
            traj = as_plane(filled(N + 1, B, n)) if with_traj else None
            ops.ode_commit_clips(torch.tensor(accept, dtype=torch.int32).cuda(), torch.tensor(ckpt, dtype=torch.int32).cuda(), as_plane(bx), as_plane(bk), x,
                                 k0, traj)
            gx, gk = as_bits(x), as_bits(k0)
            gt = as_bits(traj) if with_traj else None
            for b in range(B):
                what = f"accept={accept} ckpt={ckpt} traj={with_traj} clip {b}"
                chk.true(what + ": x", same(gx[b], bx[b]) if accept[b] else untouched(gx[b]))
                chk.true(what + ": k0", same(gk[b], bk[b]) if accept[b] else untouched(gk[b]))
                for c in range(N + 1 if with_traj else 0):
                    hit = accept[b] and ckpt[b] == c and c > 0
                    chk.true(what + f": traj[{c}]", same(gt[c, b], bx[b]) if hit else untouched(gt[c, b]))
    chk.done()


# ---- output_update and score_update: 1x1 and 3x3, bf16 and f32 -----------------------------------------------------------------------------
@pytest.mark.parametrize("ks", [1, 3])
@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_output_update(ops, chk, dtype, ks):
    """dst = base + coef (v + kold), ksave = v: exact on integer data, else within (t + 3) u (sum of magnitudes), t = 4 or 36 taps
    (solver_ops_ref.output_update_bound) -- on every border, the corners and the interior, with base / kold / ksave present or null."""
    rng = np.random.default_rng(10 + ks)
    for shape in R.IMAGE_SHAPES:
        for exact in (True, False):
            w = R.output_weights(rng, ks, exact)
            pyr, (base, kold, _, _) = R.image_data(rng, shape, dtype, exact)
            coef = 0.25 if exact else 0.0371
            dpyr, dw, dbase, dkold = nhwc(pyr, dtype), torch.from_numpy(w).cuda(), plane(base), plane(kold)
            for b_, k_, save in ((1, 1, 1), (0, 1, 1), (1, 0, 1), (1, 1, 0)):
                dst, ksave = ops.output_update(dpyr, dw, coef, base=dbase if b_ else None, kold=dkold if k_ else None, dst=nans(*shape),
                                               ksave=nans(*shape) if save else None, want_ksave=bool(save))
                hb, hk = base if b_ else None, kold if k_ else None
                ref_d, ref_k = R.output_update_ref(pyr, w, hb, hk, coef)
                bd, bk = (None, None) if exact else R.output_update_bound(pyr, w, hb, hk, coef)
                what = f"{shape} {'exact' if exact else 'random'} base={b_} kold={k_} ksave={save}"
                chk.image(what + " dst", back(dst), ref_d, bd)
                if save:
                    chk.image(what + " ksave", back(ksave), ref_k, bk)
    chk.done()


@pytest.mark.parametrize("ks", [1, 3])
@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_score_update(ops, chk, dtype, ks):
    """dst = cb base + cy Y + cn v + cz z: exact on integer data, else within (t + 3) u (sum of magnitudes); cy = 0 with NaNs in Y and
    cz = 0 with NaNs in z leave the result finite and equal to the reference without those terms."""
    rng = np.random.default_rng(20 + ks)
    for shape in R.IMAGE_SHAPES:
        for exact in (True, False):
            w = R.output_weights(rng, ks, exact)
            pyr, (base, Y, z, _) = R.image_data(rng, shape, dtype, exact)
            cb, cy, cn, cz = (0.5, -2.0, 0.25, 4.0) if exact else (0.93, 0.071, -0.013, 0.37)
            dpyr, dw, dbase, dY, dz, bad = nhwc(pyr, dtype), torch.from_numpy(w).cuda(), plane(base), plane(Y), plane(z), nans(*shape)
            for cy_, cz_, tY, tz in ((cy, cz, dY, dz), (0.0, cz, bad, dz), (cy, 0.0, dY, bad), (0.0, 0.0, None, None)):
                got = back(ops.score_update(dpyr, dw, dbase, cb, tY, cy_, cn, cz_, z=tz, dst=nans(*shape)))
                ref = R.score_update_ref(pyr, w, base, cb, Y, cy_, cn, z, cz_)
                bound = None if exact else R.score_update_bound(pyr, w, base, cb, Y, cy_, cn, z, cz_)
                chk.image(f"{shape} {'exact' if exact else 'random'} cy={cy_} cz={cz_}", got, ref, bound)
    chk.done()


@pytest.mark.parametrize("ks", [1, 3])
@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_score_update_seeded(ops, chk, dtype, ks):
    """The seeded form == the buffer form fed the plane fd_noise_fill writes for the same seeds and draw, bit for bit (draw 0 and 3, two clips
    with different seeds); the buffer form on that plane is within the bound of float64."""
    from flowdec_amd.noise import noise_fill
    rng = np.random.default_rng(30 + ks)
    seeds = seeds_of(0x1234567890ABCDEF, 42)
    for shape in ((2, 5, 7), (2, 1, 9), (2, 8, 1)):
        B, H, W = shape
        w = R.output_weights(rng, ks, False)
        pyr, (base, Y, _, _) = R.image_data(rng, shape, dtype, False)
        dpyr, dw, dbase, dY = nhwc(pyr, dtype), torch.from_numpy(w).cuda(), plane(base), plane(Y)
        for draw in (0, 3):
            zt = noise_fill(seeds, H, W, draw0=draw)[0, :, 0].contiguous()
            z = back(zt)
            chk.true("the two clips' noise planes are equal", not np.array_equal(z[0], z[1]))
            buf = back(ops.score_update(dpyr, dw, dbase, 0.93, dY, 0.071, -0.013, 0.37, z=zt, dst=nans(*shape)))
            seeded = back(ops.score_update(dpyr, dw, dbase, 0.93, dY, 0.071, -0.013, 0.37, seeds=seeds, draw=draw, dst=nans(*shape)))
            chk.true(f"{shape} draw {draw}: seeded != buffer", R.same_bits(seeded, buf))
            chk.image(f"{shape} draw {draw}", buf, R.score_update_ref(pyr, w, base, 0.93, Y, 0.071, -0.013, z, 0.37),
                      R.score_update_bound(pyr, w, base, 0.93, Y, 0.071, -0.013, z, 0.37))
    chk.done()


# ---- init_state and caxpy -----------------------------------------------------------------------------------------------------------
STATE_SHAPES = ((3, 11, 6), (2, 37, 29))      # B > 1, F != T; the second spans several blocks and has an odd T


@pytest.mark.parametrize("per_f", [False, True], ids=["sigma_n_1", "sigma_n_F"])
def test_init_state(ops, chk, per_f):
    """x0 = Y + sigma_fac * nx with nx = float32(sigma[f] * float64(z)) emulated exactly: within 2 u (|Y| + |sigma_fac nx|), and equal to
    float64 on dyadic data with sigma_fac = 1/2.  The sigma curve varies strongly with f: a wrong frequency index is far outside the bound
    (tests/test_solver_ops_cpu.py)."""
    rng = np.random.default_rng(40)
    for shape in STATE_SHAPES:
        for exact in (True, False):
            Y, z = R.plane_data(rng, shape, exact)
            sigma = R.sigma_curve(shape[1], exact)
            sigma = sigma if per_f else sigma[3:4]
            fac = 0.5 if exact else 0.731
            got = back(ops.init_state(plane(Y), torch.from_numpy(sigma).cuda(), fac, noise=plane(z), out=nans(*shape)))
            ref = R.init_state_ref(Y, sigma, fac, z)
            chk.exact(f"{shape}", got, ref) if exact else chk.bounded(f"{shape}", got, ref, R.init_state_bound(Y, sigma, fac, z))
    chk.done()


def test_init_state_seeded(ops, chk):
    """The seeded form == the buffer form on fd_noise_fill's plane, bit for bit; with frame0 = [0, 5, 12] == the buffer form on the
    fd_noise_fill_at plane, whose columns are those of a longer fd_noise_fill plane."""
    from flowdec_amd import _lib as L
    from flowdec_amd.noise import noise_fill
    rng = np.random.default_rng(41)
    seeds = seeds_of(7, 0xFEDCBA9876543210, 99)
    frame0 = torch.tensor([0, 5, 12], dtype=torch.int32).cuda()
    for B, F, T in ((3, 11, 6), (3, 9, 7)):
        Y = R.plane_data(rng, (B, F, T), False)[0]
        sigma = torch.from_numpy(R.sigma_curve(F, False)).cuda()
        dY = plane(Y)
        for draw in (0, 2):
            zt = noise_fill(seeds, F, T, draw0=draw)[0, :, 0].contiguous()
            buf = back(ops.init_state(dY, sigma, 0.731, noise=zt, out=nans(B, F, T)))
            seeded = back(ops.init_state(dY, sigma, 0.731, seeds=seeds, draw=draw, out=nans(B, F, T)))
            chk.true(f"{(B, F, T)} draw {draw}: seeded != buffer", R.same_bits(seeded, buf))
            chk.bounded(f"{(B, F, T)} draw {draw}", buf, R.init_state_ref(Y, sigma.cpu().numpy(), 0.731, back(zt)),
                        R.init_state_bound(Y, sigma.cpu().numpy(), 0.731, back(zt)))
            za = nans(B, F, T)
            L.check(L.load().fd_noise_fill_at(L.ptr(za), L.ptr(seeds), L.ptr(frame0), B, F, T, draw, 1, 0, L.stream()))
            long = noise_fill(seeds, F, T + 12, draw0=draw)[0, :, 0]
            for b, f0 in enumerate((0, 5, 12)):
                chk.true(f"fd_noise_fill_at row {b} is not the columns {f0}.. of the longer plane", R.same_bits(back(za[b]), back(long[b, :, f0:f0 + T].contiguous())))
            buf = back(ops.init_state(dY, sigma, 0.731, noise=za, out=nans(B, F, T)))
            seeded = back(ops.init_state(dY, sigma, 0.731, seeds=seeds, frame0=frame0, draw=draw, out=nans(B, F, T)))
            chk.true(f"{(B, F, T)} draw {draw} frame0: seeded != buffer", R.same_bits(seeded, buf))
    chk.done()


def test_caxpy(ops, chk):
    """dst = a + cq q: exact on integers with cq = 1/2, within 2 u (|a| + |cq q|) on random data, seeded == buffer bit for bit."""
    from flowdec_amd.noise import noise_fill
    rng = np.random.default_rng(42)
    for shape in STATE_SHAPES:
        for exact in (True, False):
            a, q = R.plane_data(rng, shape, exact)
            cq = 0.5 if exact else -1.37
            got = back(ops.caxpy(plane(a), cq, q=plane(q), out=nans(*shape)))
            ref = R.caxpy_ref(a, cq, q)
            chk.exact(f"{shape}", got, ref) if exact else chk.bounded(f"{shape}", got, ref, R.caxpy_bound(a, cq, q))
    seeds = seeds_of(5, 6)
    B, F, T = STATE_SHAPES[1]
    a = R.plane_data(rng, (B, F, T), False)[0]
    for draw in (0, 4):
        zt = noise_fill(seeds, F, T, draw0=draw)[0, :, 0].contiguous()
        buf = back(ops.caxpy(plane(a), -1.37, q=zt, out=nans(B, F, T)))
        chk.true(f"draw {draw}: seeded != buffer", R.same_bits(back(ops.caxpy(plane(a), -1.37, seeds=seeds, draw=draw, out=nans(B, F, T))), buf))
        chk.bounded(f"draw {draw}", buf, R.caxpy_ref(a, -1.37, back(zt)), R.caxpy_bound(a, -1.37, back(zt)))
    chk.done()


# ---- pack_input and combine -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_pack_input(ops, chk, dtype):
    """(x.re, x.im, y.re, y.im) rounded to the storage type in channels 0..3, zeros in 4..7, bit for bit; n = 257 and two images."""
    rng = np.random.default_rng(50)
    for shape in ((1, 1, 257), (2, 3, 43)):
        x, y = R.plane_data(rng, shape, False)
        out = torch.full(shape + (8,), float("nan"), dtype=DT[dtype], device="cuda")
        got = ops.pack_input(plane(x), plane(y), DT[dtype], out=out).float().cpu().numpy()
        chk.true(f"{shape}: placement or rounding", R.same_bits(got, R.pack_ref(x, y, dtype)))
    chk.done()


def run_combine(ops, p4, w, bias, h, dtype):
    B, H, W, Cout = h.shape
    out = torch.full((B, H, W, Cout), float("nan"), dtype=DT[dtype], device="cuda")
    stats = torch.full((B, -(-H * W // R.COMBINE_PX), Cout, 2), float("nan"), dtype=torch.float32, device="cuda")
    ops.combine(nhwc(p4, dtype), torch.from_numpy(w).cuda(), torch.from_numpy(bias).cuda(), nhwc(h, dtype), out=out, stats=stats)
    return out.float().cpu().numpy(), stats.cpu().numpy()


@pytest.mark.parametrize("Cout", R.COMBINE_COUTS)
@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_combine_exact(ops, chk, dtype, Cout):
    """Integer data: out == the integer reference, and every [b][tile][c] partial == the integer sum and sum of squares of its 256-pixel tile."""
    rng = np.random.default_rng(60 + Cout)
    for H, W in R.COMBINE_HW:
        p4, w, bias, h = R.combine_data(rng, 2, H, W, Cout, dtype, exact=True)
        out, stats = run_combine(ops, p4, w, bias, h, dtype)
        ref = R.combine_ref(p4, w, bias, h)
        chk.exact(f"HW={H * W} out", out, ref)
        s, ss, _ = R.tile_sums(ref)
        chk.exact(f"HW={H * W} sums", stats[..., 0], s)
        chk.exact(f"HW={H * W} sums of squares", stats[..., 1], ss)
    chk.done()


@pytest.mark.parametrize("Cout", R.COMBINE_COUTS)
@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_combine_random(ops, chk, dtype, Cout):
    """The stored output is within solver_ops_ref.combine_bound of float64, and the partials are the statistics of the STORED (rounded)
    values: within 256 u relative of the float64 sums of `out` itself (solver_ops_ref.stats_bound)."""
    rng = np.random.default_rng(70 + Cout)
    for H, W in R.COMBINE_HW:
        p4, w, bias, h = R.combine_data(rng, 2, H, W, Cout, dtype, exact=False)
        out, stats = run_combine(ops, p4, w, bias, h, dtype)
        chk.bounded(f"HW={H * W} out", out, R.combine_ref(p4, w, bias, h), R.combine_bound(p4, w, bias, h, dtype))
        s, ss, _ = R.tile_sums(out)
        bs, bss = R.stats_bound(out)
        chk.bounded(f"HW={H * W} sums", stats[..., 0], s, bs)
        chk.bounded(f"HW={H * W} sums of squares", stats[..., 1], ss, bss)
    chk.done()


# ---- refusals -------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_outputs_untouched(chk):
    """Every argument check of every wrapper returns FD_EINVAL with its message and launches nothing: the sentinel-filled buffer that
    stands for every pointer of the refused calls is untouched."""
    from flowdec_amd import _lib as L
    lib = L.load()
    buf = torch.from_numpy(R.sentinel(4096)).cuda()
    for dt in (L.FD_F32, L.FD_BF16):
        for label, call, msg in R.refusal_cases(lib, C.c_void_p(buf.data_ptr()), dt):
            rc = call()
            chk.true(f"{label}: returned {rc}, message {lib.fd_last_error()!r}", rc == -1 and msg in lib.fd_last_error().decode())
    torch.cuda.synchronize()
    chk.true("a refused call wrote to its buffers", bool((buf.view(torch.int32) == R.NAN_BITS).all()))
    chk.done()
