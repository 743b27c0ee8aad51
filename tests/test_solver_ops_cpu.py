"""The operator-level solver tests without a GPU: the new symbols are declared, exported and bound, their argument checks answer before
any device call, and the references and bounds of tests/solver_ops_ref.py are sound -- for every case of tests/test_hip_solver_ops.py a
float32 restatement of the kernel's formula, with the multiply-adds fused and unfused, stays within the stated bound of the float64
reference and equals it on every 'exact' data set.  A restatement outside a bound means the bound's derivation is wrong."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import solver_ops_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("fd_op_pack_input", "fd_op_combine", "fd_op_output_update", "fd_op_score_update", "fd_op_init_state", "fd_op_caxpy", "fd_op_ode_lincomb",
         "fd_op_ode_lincomb_clips", "fd_op_ode_scaled_sq", "fd_op_ode_scaled_sq_clips", "fd_op_ode_commit_clips")
FUSED = (True, False)


def test_symbols_are_declared_exported_and_bound():
    from flowdec_amd import _lib as L
    from flowdec_amd import ops
    src = open(os.path.join(ROOT, "include", "flowdec_hip.h")).read()
    assert "Operator-level: solver and edge kernels" in src
    decl = set(re.findall(r"\b(fd_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", src, flags=re.S)))
    lib = L.load()
    for name in NAMES:
        assert name in decl, f"{name} is not declared in include/flowdec_hip.h"
        assert name in L.SIGNATURES, f"{name} has no ctypes signature"
        assert getattr(lib, name).argtypes == L.SIGNATURES[name][1]
    # the section also holds the two time-conditioning entries, which tests/test_temb_cpu.py checks
    assert {n for n in decl if n.startswith("fd_op_")} == set(NAMES) | {"fd_op_time_embedding", "fd_op_temb_bias_jobs"}
    for helper in ("pack_input", "combine", "output_update", "score_update", "init_state", "caxpy", "ode_lincomb", "ode_scaled_sq", "ode_commit_clips"):
        assert callable(getattr(ops, helper))
    assert "ops_api.hip" in __import__("flowdec_amd.build", fromlist=["SOURCES"]).SOURCES


def test_build_sources_are_exactly_the_hip_files():
    """Every .hip file under csrc is linked into the library and every listed source exists: a new file cannot be left out, a deleted one
    cannot be left in."""
    from flowdec_amd import build
    on_disk = {f for f in os.listdir(build.CSRC) if f.endswith(".hip")}
    assert len(build.SOURCES) == len(set(build.SOURCES)), sorted(build.SOURCES)
    assert set(build.SOURCES) == on_disk, sorted(set(build.SOURCES) ^ on_disk)


def test_every_argument_check_refuses_before_the_device():
    from flowdec_amd import _lib as L
    lib = L.load()
    host = (C.c_float * 4096)()
    cases = R.refusal_cases(lib, C.c_void_p(C.addressof(host)), L.FD_F32)
    assert {c[0].split()[0] for c in cases} == {"pack", "combine", "output", "score", "init", "caxpy", "lincomb", "lincomb_clips", "scaled_sq",
                                                "scaled_sq_clips", "commit"}
    for label, call, msg in cases:
        assert call() == -1, f"{label}: not refused with FD_EINVAL"
        assert msg in lib.fd_last_error().decode(), f"{label}: message {lib.fd_last_error()!r}"
    assert not any(host)


# ---- the bounds are conditions the float32 arithmetic meets --------------------------------------------------------------------------
def within(got, ref, bound, what):
    ratio = R.worst_ratio(got, ref, bound)
    assert ratio <= 1.0, f"{what}: error / bound = {ratio:.3f}"
    return ratio


@pytest.mark.parametrize("fused", FUSED)
def test_lincomb_restatement(fused):
    rng = np.random.default_rng(1)
    for n in R.LINCOMB_SIZES:
        for nk in (1, 6, 7):
            x, ks, cs, dt = R.lincomb_exact_data(rng, n, nk)
            for cx in (1.0, -0.5, 0.0):
                assert R.equals_f64(R.lincomb_f32(x, cx, dt, ks, cs, fused), R.lincomb_ref(x, cx, dt, ks, cs)), (n, nk, cx)
        rows = R.dp_rows() if n <= 768 * 64 else R.dp_rows()[-2:]
        x, ks = R.lincomb_random_data(rng, n, 7)
        for name, cx, cs in rows:
            kk = ks[:len(cs)]
            for dt in (0.0371, -1.25e-3):
                within(R.lincomb_f32(x, cx, dt, kk, cs, fused), R.lincomb_ref(x, cx, dt, kk, cs), R.lincomb_bound(x, cx, dt, kk, cs), f"lincomb {name} n={n}")
    # the contracts, on the restatement: a dropped term is not read, dt = 0 with cx = 1 returns x
    x, ks = R.lincomb_random_data(rng, 257, 3)
    nan = np.full_like(x, np.nan)
    assert np.isfinite(R.lincomb_f32(nan, 0.0, 0.5, ks, [1.0, 2.0, 3.0], fused)).all()
    assert R.same_bits(R.lincomb_f32(x, 1.0, 0.5, [ks[0], nan, None], [1.0, 0.0, 3.0], fused), R.lincomb_f32(x, 1.0, 0.5, ks[:1], [1.0], fused))
    assert R.same_bits(R.lincomb_f32(x, 1.0, 0.0, ks, [1.0, 2.0, 3.0], fused), x)
    assert len(R.kept_terms(ks + ks + [ks[0]], R.dp_rows()[-1][2])) == 6          # the error row has one zero: m = 6


@pytest.mark.parametrize("fused", FUSED)
def test_scaled_sq_restatement(fused):
    rng = np.random.default_rng(2)
    for n in R.NORM_SIZES:
        for with_q in (True, False):
            p, q, r, s = R.scaled_sq_data(rng, n, exact=True)
            q = q if with_q else None
            ref = R.scaled_sq_ref(p, q, r, s, 0.125, 0.0)
            assert R.scaled_sq_f32(p, q, r, s, 0.125, 0.0, fused) == ref == float(int(ref))
            blocks = R.scaled_sq_block_ref(p, q, r, s, 0.125, 0.0)
            assert blocks.sum() == ref and not blocks[-(-n // 256):].any()
            p, q, r, s = R.scaled_sq_data(rng, n, exact=False)
            q = q if with_q else None
            for atol, rtol in ((1e-5, 1e-5), (1e-3, 0.05)):
                ref = R.scaled_sq_ref(p, q, r, s, atol, rtol)
                assert abs(R.scaled_sq_f32(p, q, r, s, atol, rtol, fused) - ref) <= R.NORM_C * R.U * ref, (n, with_q, atol)
                if n >= 2:   # the data tell max(|r|, |s|) from |r| alone: the wrong norm is far outside the bound
                    assert abs(R.scaled_sq_ref(p, q, r, s, atol, rtol, r_only=True) - ref) > 100 * R.NORM_C * R.U * ref
    assert (R.scaled_sq_block_ref(*R.scaled_sq_data(rng, 768 * 64, True), 0.125, 0.0) == 0).sum() == 512 - 192


@pytest.mark.parametrize("fused", FUSED)
@pytest.mark.parametrize("ks", (1, 3))
@pytest.mark.parametrize("dtype", ("bf16", "fp32"))
def test_output_and_score_update_restatement(dtype, ks, fused):
    rng = np.random.default_rng(3)
    for shape in R.IMAGE_SHAPES:
        for exact in (True, False):
            w = R.output_weights(rng, ks, exact)
            pyr, (base, kold, z, _) = R.image_data(rng, shape, dtype, exact)
            assert np.array_equal(pyr, R.stored(pyr, dtype))
            coef = 0.25 if exact else 0.0371
            for b_, k_ in ((base, kold), (None, kold), (base, None)):
                got = R.output_update_f32(pyr, w, b_, k_, coef, fused)
                ref, bound = R.output_update_ref(pyr, w, b_, k_, coef), R.output_update_bound(pyr, w, b_, k_, coef)
                for g, r_, bd, what in zip(got, ref, bound, ("dst", "ksave")):
                    assert R.equals_f64(g, r_) if exact else within(g, r_, bd, f"output_update {what} {shape}") <= 1
            cb, cy, cn, cz = (0.5, -2.0, 0.25, 4.0) if exact else (0.93, 0.071, -0.013, 0.37)
            for cy_, cz_ in ((cy, cz), (0.0, cz), (cy, 0.0)):
                got = R.score_update_f32(pyr, w, base, cb, kold, cy_, cn, z, cz_, fused)
                ref = R.score_update_ref(pyr, w, base, cb, kold, cy_, cn, z, cz_)
                assert R.equals_f64(got, ref) if exact else within(got, ref, R.score_update_bound(pyr, w, base, cb, kold, cy_, cn, z, cz_), "score_update") <= 1


def test_output_layer_reference_keeps_images_and_rows_apart():
    """The 3x3 reference pads every image on its own: image b's border does not see image b +- 1, and a row's ends do not see the
    neighbouring rows -- checked against a direct loop over the nine taps of one pixel."""
    rng = np.random.default_rng(4)
    w = R.output_weights(rng, 3, False)
    pyr, _ = R.image_data(rng, (3, 5, 7), "fp32", False)
    ref = R.output_layer_ref(pyr, w)
    for b, h, x in ((1, 0, 0), (1, 4, 6), (0, 4, 0), (2, 0, 6), (1, 2, 3)):
        v = np.zeros(2)
        for dy in range(3):
            for dx in range(3):
                hh, xx = h + dy - 1, x + dx - 1
                if 0 <= hh < 5 and 0 <= xx < 7:
                    v += w[:, :, dy, dx].astype(np.float64) @ pyr[b, hh, xx].astype(np.float64)
        assert np.allclose(ref[b, h, x], v, rtol=1e-14, atol=0)
    assert {k: int(m.sum()) for k, m in R.regions(5, 7).items()} == {"top": 7, "bottom": 7, "left": 5, "right": 5, "corners": 4, "interior": 15}
    assert int(R.regions(1, 9)["interior"].sum()) == 0 and int(R.regions(1, 9)["corners"].sum()) == 2


@pytest.mark.parametrize("fused", FUSED)
def test_init_state_and_caxpy_restatement(fused):
    rng = np.random.default_rng(5)
    B, F, T = 3, 11, 6
    for exact in (True, False):
        Y, z = R.plane_data(rng, (B, F, T), exact)
        fac = 0.5 if exact else 0.731
        for sigma in (R.sigma_curve(F, exact), R.sigma_curve(F, exact)[3:4]):
            got, ref = R.init_state_f32(Y, sigma, fac, z, fused), R.init_state_ref(Y, sigma, fac, z)
            assert R.equals_f64(got, ref) if exact else within(got, ref, R.init_state_bound(Y, sigma, fac, z), "init_state") <= 1
        got, ref = R.caxpy_f32(Y, fac, z, fused), R.caxpy_ref(Y, fac, z)
        assert R.equals_f64(got, ref) if exact else within(got, ref, R.caxpy_bound(Y, fac, z), "caxpy") <= 1
    # a wrong frequency index (the frame's, or a neighbouring row's) is far outside the bound
    Y, z = R.plane_data(rng, (B, F, T), False)
    sigma = R.sigma_curve(F, False)
    ref, bound = R.init_state_ref(Y, sigma, 0.731, z), R.init_state_bound(Y, sigma, 0.731, z)
    assert R.worst_ratio(R.init_state_f32(Y, np.roll(sigma, 1), 0.731, z, fused), ref, bound) > 1e3
    wrong = R.fma32(np.float32(0.731), R.f32(sigma[np.arange(T) % F][None, None, :, None] * z.astype(np.float64)), Y, fused)
    assert R.worst_ratio(wrong, ref, bound) > 1e3


@pytest.mark.parametrize("fused", FUSED)
@pytest.mark.parametrize("dtype", ("bf16", "fp32"))
def test_pack_and_combine_restatement(dtype, fused):
    rng = np.random.default_rng(6)
    x, y = R.plane_data(rng, (1, 1, 257), False)
    packed = R.pack_ref(x, y, dtype)
    assert packed.shape == (1, 1, 257, 8) and not packed[..., 4:].any() and np.array_equal(packed[..., :4], R.stored(packed[..., :4], dtype))
    for Cout in R.COMBINE_COUTS:
        for H, W in R.COMBINE_HW:
            p4, w, bias, h = R.combine_data(rng, 2, H, W, Cout, dtype, exact=True)
            out = R.combine_f32(p4, w, bias, h, dtype, fused)
            assert R.equals_f64(out, R.combine_ref(p4, w, bias, h)) and np.abs(out).max() <= 16
            s, ss = R.stats_f32(out, fused)
            rs, rss, _ = R.tile_sums(out)
            assert R.equals_f64(s, rs) and R.equals_f64(ss, rss) and rss.max() < 2 ** 17
            p4, w, bias, h = R.combine_data(rng, 2, H, W, Cout, dtype, exact=False)
            out = R.combine_f32(p4, w, bias, h, dtype, fused)
            within(out, R.combine_ref(p4, w, bias, h), R.combine_bound(p4, w, bias, h, dtype), f"combine out {dtype}")
            s, ss = R.stats_f32(out, fused)
            rs, rss, _ = R.tile_sums(out)
            bs, bss = R.stats_bound(out)
            within(s, rs, bs, "combine sum")
            within(ss, rss, bss, "combine sum of squares")
            if dtype == "bf16":   # statistics taken before the rounding are outside the bound: the test tells the two apart
                unrounded = R.combine_f32(p4, w, bias, h, "fp32", fused)
                assert R.worst_ratio(R.tile_sums(unrounded)[1], rss, bss) > 1
