"""The operator-level time-conditioning tests without a GPU: the symbols are declared, exported and bound, every argument check answers
before any device call, and the references and bounds of tests/temb_ref.py are sound -- on the exact inputs of tests/test_hip_temb.py a
float32 restatement of each kernel's operation order, with the multiply-adds fused and unfused, stays within the counted bound of the
float64 reference.  A restatement outside a bound means the bound's derivation is wrong; a mistake the GPU tests are meant to catch
(another rounding of pi, swapped halves, a dropped term) must fall outside it."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import temb_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("fd_op_time_embedding", "fd_op_temb_bias_jobs")
FUSED = (True, False)


def within(got, ref, bound, what):
    ratio = R.worst_ratio(got, ref, bound)
    assert ratio <= 1.0, f"{what}: error / bound = {ratio:.3f}"
    return ratio


def test_symbols_are_declared_exported_and_bound():
    from flowdec_amd import _lib as L
    from flowdec_amd import ops
    src = open(os.path.join(ROOT, "include", "flowdec_hip.h")).read()
    decl = set(re.findall(r"\b(fd_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", src, flags=re.S)))
    lib = L.load()
    for name in NEW + ("fd_time_embedding", "fd_temb_bias"):
        assert name in decl, f"{name} is not declared in include/flowdec_hip.h"
        assert name in L.SIGNATURES, f"{name} has no ctypes signature"
        assert getattr(lib, name).argtypes == L.SIGNATURES[name][1]      # AttributeError: the library does not export it
    for helper in ("time_embedding", "temb_bias", "op_time_embedding", "temb_bias_jobs"):
        assert callable(getattr(ops, helper))
    doc = src[src.index("Operator-level: solver and edge kernels"):src.index("Front / back end")]
    assert all(name in doc for name in NEW), "the new entries are not documented in the header's Operator-level section"


def test_every_argument_check_refuses_before_the_device():
    from flowdec_amd import _lib as L
    lib = L.load()
    host = (C.c_float * 4096)()
    base = C.addressof(host)
    cases = R.refusal_cases(lib, C.c_void_p(base + (-base) % 16))
    assert {c[0].split()[0] for c in cases} == {"fd_time_embedding", "fd_op_time_embedding", "fd_temb_bias", "fd_op_temb_bias_jobs"}
    for label, call, msg in cases:
        assert call() == -1, f"{label}: not refused with FD_EINVAL ({lib.fd_last_error()!r})"
        err = lib.fd_last_error().decode()
        assert err.startswith(label.split()[0] + ": ") and msg in err, f"{label}: message {err!r}"
    assert not any(host)


def test_case_lists_cover_what_the_kernels_branch_on():
    assert {c[1] for c in R.embedding_cases()} == set(R.NFS) and {c[2] for c in R.embedding_cases()} == set(R.NTS)
    assert {(nf, nt) for _, nf, nt, reach in R.embedding_cases() if reach is None} == {(nf, nt) for nf in R.NFS for nt in R.NTS}
    for nt in R.NTS:
        assert {c[0] for c in R.bias_cases() if c[2] == nt} == set(R.TEMB_DIMS) and {c[1] for c in R.bias_cases() if c[2] == nt} == set(R.COUTS)
    assert {(D, Co) for D, Co, nt in R.bias_cases() if nt == 3} == {(D, Co) for D in R.TEMB_DIMS for Co in R.COUTS}
    assert set(R.job_couts(R.NJOBS)) == set(R.COUTS)
    t = R.times(256, np.random.default_rng(0))
    assert t[0] == np.float32(R.T_MIN) and t[1] == 1 and t[2] == 0 and 0 <= t.min() and t.max() <= 1
    _, W, *_ = R.embedding_inputs(128, 3, 2000.0)
    assert abs(np.abs(R.angle32([1.0], W)).max() - 2000.0) < 1.0
    _, W, *_ = R.embedding_inputs(128, 3)
    assert np.abs(R.angle32([1.0], W)).max() > 200.0                 # several hundred radians at the checkpoints' scale
    x = R.bias_inputs(256, 8, 3)[0]
    assert x.min() == -12 and x.max() == 12


def test_silu_restatement_and_bound():
    """fd_silu restated in float32 against float64 over [-80, 80], the log2e term included: the restatement stays within the counted budget,
    and a budget without the |x|-proportional term would not hold it (so the term is needed, not decoration)."""
    x = np.concatenate([np.linspace(-80, 80, 200001), np.linspace(-12, 12, 200001), [0.0, 12.0, -12.0]]).astype(np.float32)
    got, ref = R.silu32(x), R.silu64(x)
    within(got, ref, R.silu_bound(x), "silu32")
    one_minus_s = 1.0 / (1.0 + np.exp(x.astype(np.float64)))
    without = (one_minus_s * 2.0 + 5.0) * R.U * np.abs(ref)
    assert R.worst_ratio(got, ref, without) > 1.0
    assert R.SILU_LIP >= np.abs(np.gradient(R.silu64(np.linspace(-20, 20, 400001)), 1e-4)).max()
    with pytest.raises(AssertionError):
        R.silu_bound(np.asarray([81.0]))


@pytest.mark.parametrize("fused", FUSED)
@pytest.mark.parametrize("label,nf,nt,reach", R.embedding_cases(), ids=[c[0] for c in R.embedding_cases()])
def test_time_embedding_restatement(label, nf, nt, reach, fused):
    args = R.embedding_inputs(nf, nt, reach)
    ref, bound = R.time_embedding_ref(*args)["temb"], R.time_embedding_bound(*args)["temb"]
    ratio = within(R.time_embedding_f32(*args, fused), ref, bound, label)
    assert ratio > 0 and bound.min() > 0


def test_time_embedding_bound_tells_the_planted_mistakes():
    """What the GPU test must catch is outside the bound in the reference's own arithmetic: pi rounded to the neighbouring float32, the
    sin and cos halves swapped, the last input of a chain dropped, a neighbouring weight row."""
    for nf in (24, 128):
        t, W, w1, b1, w2, b2 = args = R.embedding_inputs(nf, 3)
        ref, bound = R.time_embedding_ref(*args)["temb"], R.time_embedding_bound(*args)["temb"]
        other_pi = R.mul32(R.mul32(R.mul32(t.reshape(-1, 1), W.reshape(1, -1)), np.float32(2.0)), np.nextafter(R.PI32, np.float32(0)))
        # the neighbouring float32 of pi moves an angle of 500 rad by 4e-5: far below the worst-case bound of two dense layers, far above
        # the bound of the one-hot probe, whose rows cost two roundings
        E, D, z = 2 * nf, 4 * nf, np.zeros(4 * nf, np.float32)
        probe = (t, W, R.onehot(D, E, R.probe_sel(D, E)), z, R.onehot(D, D), z)
        assert R.worst_ratio(R.time_embedding_ref(*probe, xp=other_pi)["temb"], R.time_embedding_ref(*probe)["temb"], R.time_embedding_bound(*probe)["temb"]) > 10
        assert R.worst_ratio(R.time_embedding_ref(*args, xp=(R.angle32(t, W).astype(np.float64) + np.pi / 2))["temb"], ref, bound) > 10    # sin <-> cos (up to sign)
        w1d = w1.copy(); w1d[:, -1] = 0
        assert R.worst_ratio(R.time_embedding_ref(t, W, w1d, b1, w2, b2)["temb"], ref, bound) > 10
        assert R.worst_ratio(R.time_embedding_ref(t, W, w1, b1, np.roll(w2, 1, 0), b2)["temb"], ref, bound) > 10


@pytest.mark.parametrize("nf", R.PROBE_NFS)
def test_index_probes_have_one_element_structure(nf):
    """With one-hot w1 (b1 = 0) the reference's hid[o] is silu of exactly emb[sel[o]]; with one-hot w2 (b2 = 0) temb[o] is exactly hid[sel[o]];
    every input index is picked, and no row picks its own index everywhere (not the identity)."""
    E, D = 2 * nf, 4 * nf
    t, W, w1, b1, w2, b2 = R.embedding_inputs(nf, 3)
    z = np.zeros(D, np.float32)
    s1, s2 = R.probe_sel(D, E), R.probe_sel(D, D)
    assert set(s1) == set(range(E)) and set(s2) == set(range(D)) and (s2 != np.arange(D)).all() and (s1[:E] != np.arange(E)).any()
    r = R.time_embedding_ref(t, W, R.onehot(D, E, s1), z, R.onehot(D, D), z)
    assert np.array_equal(r["h"], r["emb"][:, s1]) and np.array_equal(r["temb"], R.silu64(r["emb"][:, s1]))
    r = R.time_embedding_ref(t, W, w1, b1, R.onehot(D, D, s2), z)
    assert np.array_equal(r["temb"], r["hid"][:, s2])
    # the columns differ from one another: a wrong index is a wrong value (the sin / cos halves included)
    emb = R.time_embedding_ref(t, W, w1, b1, w2, b2)["emb"][1]
    assert len(np.unique(emb)) == E
    for D_ in R.TEMB_DIMS:
        sel = R.probe_sel(D_ + 1, D_)
        assert set(sel) == set(range(D_)) and (sel[:D_] != np.arange(D_)).all()
        x = R.temb_rows(1, 3, D_)
        assert np.array_equal(R.temb_bias_ref(x, R.onehot(D_ + 1, D_, sel), np.zeros(D_ + 1, np.float32), None), R.silu64(x)[:, sel])


@pytest.mark.parametrize("fused", FUSED)
@pytest.mark.parametrize("D,Cout,nt", R.bias_cases())
def test_temb_bias_restatement(D, Cout, nt, fused):
    temb, dw, db, cb = R.bias_inputs(D, Cout, nt)
    for c in (cb, None):
        within(R.temb_bias_f32(temb, dw, db, c, fused), R.temb_bias_ref(temb, dw, db, c), R.temb_bias_bound(temb, dw, db, c), f"D={D} Cout={Cout} nt={nt}")
    if fused:   # a dropped conv bias, a neighbouring time row and a dropped last term are far outside the bound
        ref, bound = R.temb_bias_ref(temb, dw, db, cb), R.temb_bias_bound(temb, dw, db, cb)
        assert R.worst_ratio(R.temb_bias_ref(temb, dw, db, None), ref, bound) > 10
        dwd = dw.copy(); dwd[:, -1] = 0
        assert R.worst_ratio(R.temb_bias_ref(temb, dwd, db, cb), ref, bound) > 10
        if nt > 1:
            assert R.worst_ratio(R.temb_bias_ref(np.roll(temb, 1, 0), dw, db, cb), ref, bound) > 10


def test_reference_matches_the_golden_fixture():
    """The float64 reference against the REFERENCE implementation's own float32 modules (tests/golden/make_golden_temb.py): the inputs
    regenerate to the recorded checksum, and the fixture -- float32 arithmetic in another summation order -- is within the counted bound."""
    g = np.load(os.path.join(ROOT, "tests", "golden", "g34_temb.npz"))
    for nf in R.GOLDEN_NFS:
        i = R.golden_inputs(nf)
        assert R.checksum(i) == int(g[f"nf{nf}_checksum"])
        args = tuple(i[k] for k in ("t", "W", "w1", "b1", "w2", "b2"))
        fix = g[f"nf{nf}_temb"]
        within(fix, R.time_embedding_ref(*args)["temb"], R.time_embedding_bound(*args)["temb"], f"nf{nf} temb")
        within(g[f"nf{nf}_bias"], R.temb_bias_ref(fix, i["dw"], i["db"], i["cb"]), R.temb_bias_bound(fix, i["dw"], i["db"], i["cb"]), f"nf{nf} bias")
