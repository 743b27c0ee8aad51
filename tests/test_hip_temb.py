"""The time-conditioning kernels at model widths, one at a time, on the GPU: time_embedding_kernel (Fourier features -> Linear -> SiLU ->
Linear), temb_bias_kernel (the batched jobs x rows table of every ResBlock's Conv_0.bias + Dense_0(silu(temb))) and its one-job form
temb_bias_single_kernel (csrc/net_edges.hip), through fd_time_embedding, fd_temb_bias and the operator-level entries
fd_op_time_embedding and fd_op_temb_bias_jobs (csrc/ops_api.hip), which call the launchers the model calls.

Every reference is NumPy float64 taken from the float32 angle, every bound is counted from the operations (tests/temb_ref.py;
tests/test_temb_cpu.py shows that float32 arithmetic itself meets them on these very inputs), every output lies between sentinel guards
and is prefilled with the sentinel, and every comparison is per element.  The dense cases hold the kernels to the worst-case bound of two
(or one) matrix-vector products; the index probes -- one-hot weight rows, whose chains cost two roundings -- are exact in their indices
and hold the values to the sin / cos and SiLU allowances alone.  The one measured number per test, the worst error / bound, goes to the
parity report."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import solver_ops_ref as S
import temb_ref as R
from test_hip_solver_ops import Check     # bounded / true / done: the worst error / bound of a test, written to the parity report

pytestmark = pytest.mark.gpu

GUARD = 64     # sentinel floats in front of and behind every output


@pytest.fixture
def chk(request):
    return Check("temb." + request.node.name.replace("test_", "", 1))


@pytest.fixture(scope="module")
def ops():
    from flowdec_amd import ops as _ops
    return _ops


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()


def guarded(rows, cols):
    """-> (buffer, view [rows][cols] inside it): all sentinel, GUARD floats on either side of the view."""
    buf = dev(S.sentinel(rows * cols + 2 * GUARD))
    return buf, buf[GUARD:GUARD + rows * cols].view(rows, cols)


def guards_intact(buf):
    b = buf.view(torch.int32)
    return bool((b[:GUARD] == S.NAN_BITS).all() and (b[-GUARD:] == S.NAN_BITS).all())


def embed(ops, chk, what, d, nt, D, t=None):
    """fd_op_time_embedding on device weights d = (W, w1, b1, w2, b2) into a guarded output -> float32 [nt][D] on the host."""
    buf, out = guarded(nt, D)
    ops.op_time_embedding(t, *d, out=out)
    got = out.cpu().numpy()
    chk.true(f"{what}: wrote outside temb [nt][4 nf]", guards_intact(buf))
    return got


# ---- time embedding against the counted bound -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("label,nf,nt,reach", R.embedding_cases(), ids=[c[0] for c in R.embedding_cases()])
def test_time_embedding_bound(ops, chk, label, nf, nt, reach):
    """|temb - ref| <= temb_ref.time_embedding_bound per element, at E = 4 .. 256 and D = 8 .. 512 (one vector; a partial first chunk; a
    partial chunk with D below the block; whole chunks with D the block; the second trip of the output loop), nt = 1, 3, 256, times 0, 1,
    the smallest solver time and uniform ones, W = 16 N(0, 1) and W reaching 2000 rad.  fd_time_embedding gives the same bits."""
    args = R.embedding_inputs(nf, nt, reach)
    t, d = dev(args[0]), [dev(a) for a in args[1:]]
    got = embed(ops, chk, label, d, nt, 4 * nf, t)
    chk.bounded(label, got, R.time_embedding_ref(*args)["temb"], R.time_embedding_bound(*args)["temb"])
    chk.true("fd_time_embedding differs from fd_op_time_embedding", S.same_bits(ops.time_embedding(t, *d).cpu().numpy(), got))
    chk.done()


@pytest.mark.parametrize("nf", R.NFS)
def test_scalar_time_path(ops, chk, nf):
    """t == NULL with t_imm = tau (the path of every fixed-step solver) == t = [tau], bit for bit; row r of an nt-row call == the nt = 1
    call on t[r], bit for bit (nt = 3: every row; nt = 256: rows across the grid)."""
    for nt, rows in ((3, (0, 1, 2)), (256, (0, 1, 2, 3, 100, 255))):
        args = R.embedding_inputs(nf, nt)
        t, d = dev(args[0]), [dev(a) for a in args[1:]]
        full = embed(ops, chk, f"nt={nt}", d, nt, 4 * nf, t)
        for r in rows:
            one = embed(ops, chk, f"nt={nt} row {r} alone", d, 1, 4 * nf, t[r:r + 1])
            imm = embed(ops, chk, f"nt={nt} row {r} by value", d, 1, 4 * nf, float(args[0][r]))
            chk.true(f"nt={nt}: row {r} differs from the one-row call", S.same_bits(one[0], full[r]))
            chk.true(f"nt={nt}: t_imm = t[{r}] differs from t = [t[{r}]]", S.same_bits(imm, one))
    chk.done()


# ---- index probes ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reach", [None, 2000.0], ids=["W16", "2000rad"])
@pytest.mark.parametrize("nf", R.PROBE_NFS)
def test_time_embedding_index_probes(ops, chk, nf, reach):
    """One-hot w1 (b1 = 0) under an identity w2: temb[o] = silu(emb[sel[o]]) for sel = (5 o + 3) mod E, every k in [0, E) picked.  One-hot w2
    (b2 = 0) under a dense w1: temb[o] == hid[sel[o]] bit for bit, hid taken from the identity-w2 run, which is itself held to the bound of
    hid.  A dropped or doubled vector at a chunk edge, swapped sin / cos halves, a wrong row stride or another rounding of pi is an error
    of one element far above these bounds (two roundings per chain, 4 ulp of sin / cos, the SiLU count)."""
    E, D = 2 * nf, 4 * nf
    t, W, w1, b1, w2, b2 = R.embedding_inputs(nf, 3, reach)
    z, s1, s2 = np.zeros(D, np.float32), R.probe_sel(D, E), R.probe_sel(D, D)
    run = lambda a: embed(ops, chk, "probe", [dev(x) for x in a[1:]], 3, D, dev(a[0]))
    a = (t, W, R.onehot(D, E, s1), z, R.onehot(D, D), z)
    chk.bounded("w1 one-hot: temb[o] = silu(emb[sel[o]])", run(a), R.time_embedding_ref(*a)["temb"], R.time_embedding_bound(*a)["temb"])
    a = (t, W, w1, b1, R.onehot(D, D), z)
    hid = run(a)
    chk.bounded("w2 identity: temb = hid", hid, R.time_embedding_ref(*a)["hid"], R.time_embedding_bound(*a)["temb"])
    chk.true("w2 one-hot: temb[o] is not hid[sel[o]]", S.same_bits(run((t, W, w1, b1, R.onehot(D, D, s2), z)), hid[:, s2]))
    chk.done()


@pytest.mark.parametrize("D", R.TEMB_DIMS)
def test_temb_bias_index_probe(ops, chk, D):
    """One-hot dense_w with dense_b = conv_b = 0, Cout = D + 1: out[r][o] = silu(temb[r][sel[o]]) within the SiLU count (+ two roundings),
    every k in [0, D) picked; the batched kernel gives the same bits."""
    Cout, nt = D + 1, 3
    temb, dw, z = R.temb_rows(R.seed_of("probe", D), nt, D), R.onehot(D + 1, D, R.probe_sel(D + 1, D)), np.zeros(D + 1, np.float32)
    dt, ddw, dz = dev(temb), dev(dw), dev(z)
    buf, out = guarded(nt, Cout)
    got = ops.temb_bias(dt, ddw, dz, dz, out=out).cpu().numpy()
    chk.bounded("single", got, R.temb_bias_ref(temb, dw, z, z), R.temb_bias_bound(temb, dw, z, z))
    buf2, out2 = guarded(nt, Cout)
    ops.temb_bias_jobs(dt, [(ddw, dz, dz, out2)])
    chk.true("batched differs from single", S.same_bits(out2.cpu().numpy(), got))
    chk.true("wrote outside out [nt][Cout]", guards_intact(buf) and guards_intact(buf2))
    chk.done()


# ---- temb bias: single and batched against the counted bound -----------------------------------------------------------------------------------
@pytest.mark.parametrize("D,Cout,nt", R.bias_cases())
def test_temb_bias_bound(ops, chk, D, Cout, nt):
    """|out - ref| <= temb_ref.temb_bias_bound per element with |temb| up to 12; a NULL conv_bias == a zero conv_bias bit for bit; the batched
    kernel with this one job == the single kernel bit for bit."""
    temb, dw, db, cb = R.bias_inputs(D, Cout, nt)
    dt, ddw, ddb, dcb = (dev(a) for a in (temb, dw, db, cb))
    outs = {}
    for name, c in (("cb", dcb), ("null", None), ("zero", torch.zeros_like(dcb))):
        buf, out = guarded(nt, Cout)
        outs[name] = ops.temb_bias(dt, ddw, ddb, c, out=out).cpu().numpy()
        chk.true(f"conv_bias {name}: wrote outside out [nt][Cout]", guards_intact(buf))
    chk.bounded("with conv_bias", outs["cb"], R.temb_bias_ref(temb, dw, db, cb), R.temb_bias_bound(temb, dw, db, cb))
    chk.bounded("conv_bias NULL", outs["null"], R.temb_bias_ref(temb, dw, db, None), R.temb_bias_bound(temb, dw, db, None))
    # x + 0.f has the bits of x for every x but -0 (which becomes +0): on results that are all nonzero the two forms cannot differ
    chk.true("a result is zero: the data cannot tell NULL from a zero conv_bias", bool((outs["null"] != 0).all()))
    chk.true("conv_bias NULL differs from a zero conv_bias", S.same_bits(outs["null"], outs["zero"]))
    buf, out = guarded(nt, Cout)
    ops.temb_bias_jobs(dt, [(ddw, ddb, dcb, out)])
    chk.true("njobs = 1 differs from fd_temb_bias", S.same_bits(out.cpu().numpy(), outs["cb"]) and guards_intact(buf))
    chk.done()


@pytest.mark.parametrize("D,nt", [(256, 3), (96, 1), (512, 256)])
def test_temb_bias_jobs(ops, chk, D, nt):
    """22 jobs of mixed Cout in one launch, their outputs in one pool with sentinel gaps: job j, row r == fd_temb_bias on that job alone, bit
    for bit; every job is within the bound; no gap is written."""
    couts = R.job_couts(R.NJOBS)
    temb = R.temb_rows(R.seed_of("jobs", D, nt), nt, D)
    params = [R.dense_params(R.seed_of("job", D, j), D, c) for j, c in enumerate(couts)]
    dt = dev(temb)
    dparams = [tuple(dev(a) for a in p) for p in params]
    offs = np.cumsum([GUARD] + [nt * c + GUARD for c in couts])
    pool = dev(S.sentinel(int(offs[-1])))
    views = [pool[int(o):int(o) + nt * c].view(nt, c) for o, c in zip(offs[:-1], couts)]
    ops.temb_bias_jobs(dt, [p + (v,) for p, v in zip(dparams, views)])
    written = torch.zeros(pool.numel(), dtype=torch.bool, device="cuda")
    for j, (c, v, p, dp) in enumerate(zip(couts, views, params, dparams)):
        got = v.cpu().numpy()
        written[int(offs[j]):int(offs[j]) + nt * c] = True
        chk.true(f"job {j} (Cout {c}) differs from fd_temb_bias on the job alone", S.same_bits(got, ops.temb_bias(dt, *dp).cpu().numpy()))
        chk.bounded(f"job {j} (Cout {c})", got, R.temb_bias_ref(temb, *p), R.temb_bias_bound(temb, *p))
    chk.true("a job wrote outside its own [nt][Cout] block", bool((pool.view(torch.int32)[~written] == S.NAN_BITS).all()))
    chk.done()


# ---- the reference implementation's own modules ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nf", R.GOLDEN_NFS)
def test_reference_anchor(ops, chk, nf):
    """Against tests/golden/g34_temb.npz (the reference's GaussianFourierProjection, Linear layers and Dense_0 in float32, nf 64 and 128):
    |got - fixture| <= counted bound + |float64 reference - fixture| per element; the bias kernels are fed the fixture's own temb."""
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g34_temb.npz"))
    i = R.golden_inputs(nf)
    chk.true("the inputs do not regenerate to the fixture's checksum", R.checksum(i) == int(g[f"nf{nf}_checksum"]))
    args = tuple(i[k] for k in ("t", "W", "w1", "b1", "w2", "b2"))
    fix = g[f"nf{nf}_temb"]
    got = embed(ops, chk, "golden", [dev(a) for a in args[1:]], 8, 4 * nf, dev(args[0]))
    ref = R.time_embedding_ref(*args)["temb"]
    chk.bounded("temb", got, fix.astype(np.float64), R.time_embedding_bound(*args)["temb"] + np.abs(ref - fix))
    fixb, refb = g[f"nf{nf}_bias"], R.temb_bias_ref(fix, i["dw"], i["db"], i["cb"])
    boundb = R.temb_bias_bound(fix, i["dw"], i["db"], i["cb"]) + np.abs(refb - fixb)
    buf, out = guarded(8, R.GOLDEN_COUT)
    dp = [dev(i[k]) for k in ("dw", "db", "cb")]
    chk.bounded("bias, single", ops.temb_bias(dev(fix), *dp, out=out).cpu().numpy(), fixb.astype(np.float64), boundb)
    buf2, out2 = guarded(8, R.GOLDEN_COUT)
    ops.temb_bias_jobs(dev(fix), [tuple(dp) + (out2,)])
    chk.bounded("bias, batched", out2.cpu().numpy(), fixb.astype(np.float64), boundb)
    chk.true("wrote outside out", guards_intact(buf) and guards_intact(buf2))
    chk.done()


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_outputs_untouched(chk):
    """Every argument check of the four entry points returns FD_EINVAL with a message that names the entry point and the argument, and
    launches nothing: the sentinel-filled buffer that stands for every pointer of the refused calls is untouched."""
    from flowdec_amd import _lib as L
    lib = L.load()
    buf = dev(S.sentinel(1 << 16))
    assert buf.data_ptr() % 16 == 0
    for label, call, msg in R.refusal_cases(lib, C.c_void_p(buf.data_ptr())):
        rc = call()
        err = lib.fd_last_error().decode()
        chk.true(f"{label}: returned {rc}, message {err!r}", rc == -1 and err.startswith(label.split()[0] + ": ") and msg in err)
    torch.cuda.synchronize()
    chk.true("a refused call wrote to its buffers", bool((buf.view(torch.int32) == S.NAN_BITS).all()))
    chk.done()
