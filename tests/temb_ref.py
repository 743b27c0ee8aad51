"""References, data and error bounds of the operator-level tests of the time-conditioning kernels (tests/test_hip_temb.py on the GPU,
tests/test_temb_cpu.py without one; include/flowdec_hip.h fd_time_embedding, fd_temb_bias, fd_op_time_embedding, fd_op_temb_bias_jobs;
csrc/net_edges.hip time_embedding_kernel, temb_bias_kernel, temb_bias_single_kernel).

The reference is NumPy float64 TAKEN FROM THE FLOAT32 ANGLE: xp = fl(fl(fl(t W) 2) pi32) in the kernel's three float32 roundings (the
doubling is exact), then sin / cos, both Linear layers, the SiLU and the bias sums in float64.  With W ~ 16 N(0, 1) the angles reach
several hundred radians, where one float32 ulp of the angle is about 3e-5: a reference from the float64 angle would need a tolerance
that hides everything else.

Bounds, per output element, counted from the operations, u = 2^-24, gamma_n = n u / (1 - n u):
  sinf / cosf   HIP's accurate device functions (no fast-math).  4 ulp, what the OpenCL full profile grants sin and cos and what the device
                library is built to; |sin|, |cos| <= 1, so 4 u absolute.
  fd_row_dot    a k-ordered chain of n fused multiply-adds started from the bias: gamma_n (|b| + sum |w| |x|).  The bounds take gamma_(n+1):
                they then also hold for a product rounded before the sum (the CPU test runs both restatements).  n counts the NONZERO
                weights of the row (a zero weight adds an exact zero).  Errors of the inputs x pass through sum |w| dx.
  fd_silu       x * v_rcp_f32(1 + __expf(-x)), __expf(y) = v_exp_f32(y * log2e).  The CDNA material this project works from does not state the
                accuracy of v_exp_f32 and v_rcp_f32: 1 ulp each is ASSUMED here (2 u relative), the figure the comments of csrc/common.h
                and tests/test_hip_fir.py use as well.  Relative to silu(x), in units of u, with s = sigmoid(x):
                  the float constant log2e (u) and the product's rounding (u) move the exponent by 2 u |x| log2e: exp(-x) by the factor
                  2 |x| u -- this term GROWS with |x| and is carried, not assumed small; v_exp_f32 2; together (2 |x| + 2) on exp(-x),
                  which enters 1 + exp(-x) with the weight exp(-x) / (1 + exp(-x)) = 1 - s;  the addition 1;  v_rcp_f32 2;  x * r 1:
                  E(x) = (1 - s) (2 |x| + 2) + 4, and + 1 for the second order.
                An input error dx passes through |silu'| <= 1.1 (the maximum of s (1 + x (1 - s)) is 1.0998).
                Domain |x| <= 80: beyond it exp(-x) leaves the float32 range and the count above does not apply.
No bound here is fitted to what a GPU returns; tests/test_temb_cpu.py shows that float32 arithmetic itself meets them.
"""
import ctypes as C
import zlib

import numpy as np

from solver_ops_ref import F64, U, add32, f32, fma32, mul32, sentinel, worst_ratio  # noqa: F401  (re-exported for the tests)

PI32 = np.float32(3.14159274101257324)
LOG2E32 = np.float32(1.4426950408889634)
ULP_SINCOS = 4.0            # ulp allowed to sinf / cosf (OpenCL full profile)
ULP_EXP, ULP_RCP = 1.0, 1.0  # ulp ASSUMED for v_exp_f32 / v_rcp_f32 (module docstring)
SILU_LIP = 1.1
SILU_DOMAIN = 80.0

NFS = (2, 8, 24, 64, 128)                 # E = 2 nf = 4 .. 256, D = 4 nf = 8 .. 512
NTS = (1, 3, 256)                         # 256 = fd_model::MAX_NT
T_MIN = 3e-2                              # the smallest solver time of the presets (t_eps of the score models)
TEMB_DIMS = (4, 32, 96, 256, 512)
COUTS = (1, 8, 33, 256, 257, 512)
NJOBS = 22                                # the ResBlocks of the default backbone
PROBE_NFS = (24, 128)


def gamma(n):
    return n * U / (1.0 - n * U)


# ---- SiLU ---------------------------------------------------------------------------------------------------------------------------------
def silu64(x):
    x = np.asarray(x, F64)
    return x / (1.0 + np.exp(-x))


def silu_units(x):
    """E(x) + 1 of the module docstring: the relative error of fd_silu(x) in units of u, for an exactly given x."""
    x = np.asarray(x, F64)
    assert np.all(np.abs(x) <= SILU_DOMAIN), "fd_silu's operation count holds for |x| <= 80"
    one_minus_s = 1.0 / (1.0 + np.exp(x))
    return one_minus_s * (2.0 * np.abs(x) + 2.0 * ULP_EXP) + 1.0 + 2.0 * ULP_RCP + 1.0 + 1.0


def silu_bound(x, dx=0.0):
    """|fd_silu(x^) - silu(x)| for |x^ - x| <= dx: 1.1 dx + (E + 1) u |silu|, the units taken as the largest of x and x +- dx."""
    x = np.asarray(x, F64)
    units = np.maximum(silu_units(x), np.maximum(silu_units(x - dx), silu_units(x + dx)))
    return SILU_LIP * dx + units * U * (np.abs(silu64(x)) + SILU_LIP * dx)


def silu32(x):
    """fd_silu restated in float32: x * (1 / (1 + exp2(-x * log2e))), every step rounded (NumPy's exp2 and division are within the allowances)."""
    x = np.asarray(x, np.float32)
    e = np.exp2(mul32(-x, LOG2E32)).astype(np.float32)
    return mul32(x, (np.float32(1.0) / add32(np.float32(1.0), e)).astype(np.float32))


# ---- the dot product of fd_row_dot -------------------------------------------------------------------------------------------------------
def row_dot32(w, x, b, fused):
    """[rows][n] x [n_out][n] -> [rows][n_out] float32: acc = b, then acc = fma(w[o][k], x[r][k], acc) for k ascending."""
    acc = np.broadcast_to(np.asarray(b, np.float32), (x.shape[0], w.shape[0])).copy()
    for k in range(w.shape[1]):
        acc = fma32(w[None, :, k], x[:, k:k + 1], acc, fused)
    return acc


def dot_bound(w, b, xabs, dx, extra=0):
    """gamma_(m + 1 + extra) (|b| + |w| (|x| + dx)) + |w| dx for x [rows][n] (magnitudes `xabs`, input errors `dx`), w [n_out][n], with m the
    NONZERO weights of the output's row: fma(0, x, acc) returns acc exactly, so a zero weight costs no rounding (for a dense row m = n; for
    the one-hot rows of the index probes m = 1, which is what makes the probes sharp in value as well as exact in index)."""
    aw = np.abs(np.asarray(w, F64))
    m = np.count_nonzero(aw, axis=1)
    return gamma(m + 1 + extra) * (np.abs(np.asarray(b, F64)) + (xabs + dx) @ aw.T) + dx @ aw.T


# ---- time embedding -----------------------------------------------------------------------------------------------------------------------
def angle32(t, W):
    """xp [nt][nf] in float32, the kernel's roundings: ((t W) 2) pi32."""
    t, W = np.asarray(t, np.float32).reshape(-1, 1), np.asarray(W, np.float32).reshape(1, -1)
    return mul32(mul32(mul32(t, W), np.float32(2.0)), PI32)


def time_embedding_ref(t, W, w1, b1, w2, b2, xp=None):
    """-> dict(emb [nt][2nf], h, hid, temb [nt][4nf]) in float64 from the float32 angle (xp: another angle, for the tests' own checks)."""
    xp = angle32(t, W).astype(F64) if xp is None else np.asarray(xp, F64)
    emb = np.concatenate([np.sin(xp), np.cos(xp)], -1)
    h = emb @ w1.astype(F64).T + b1.astype(F64)
    hid = silu64(h)
    return dict(emb=emb, h=h, hid=hid, temb=hid @ w2.astype(F64).T + b2.astype(F64))


def time_embedding_bound(t, W, w1, b1, w2, b2):
    """-> dict(hid, temb): the bounds of the module docstring chained through the three stages."""
    r = time_embedding_ref(t, W, w1, b1, w2, b2)
    demb = np.full_like(r["emb"], ULP_SINCOS * U)
    dh = dot_bound(w1, b1, np.abs(r["emb"]), demb)
    dhid = silu_bound(r["h"], dh)
    return dict(hid=dhid, temb=dot_bound(w2, b2, np.abs(r["hid"]), dhid))


def time_embedding_f32(t, W, w1, b1, w2, b2, fused):
    xp = angle32(t, W)
    emb = np.concatenate([np.sin(xp), np.cos(xp)], -1).astype(np.float32)
    return row_dot32(w2, silu32(row_dot32(w1, emb, b1, fused)), b2, fused)


def times(nt, rng):
    """[nt] float32: the smallest solver time, 1, 0, then seeded uniform values."""
    return np.concatenate([[T_MIN, 1.0, 0.0], rng.uniform(0.0, 1.0, max(nt - 3, 0))])[:nt].astype(np.float32)


def temb_weights(seed, nf, reach=None):
    """W [nf] = 16 N(0, 1) (reach: scaled so that 2 pi max |W| = reach radians at t = 1), w1 [4nf][2nf], b1, w2 [4nf][4nf], b2; float32."""
    rng = np.random.default_rng(seed)
    E, D = 2 * nf, 4 * nf
    W = 16.0 * rng.standard_normal(nf)
    if reach is not None:
        W = W * (reach / (2.0 * np.pi * np.abs(W).max()))
    w1, b1 = rng.standard_normal((D, E)) / np.sqrt(E), 0.3 * rng.standard_normal(D)
    w2, b2 = rng.standard_normal((D, D)) / np.sqrt(D), 0.3 * rng.standard_normal(D)
    return tuple(np.ascontiguousarray(a, np.float32) for a in (W, w1, b1, w2, b2))


# ---- index probes -------------------------------------------------------------------------------------------------------------------------
def probe_sel(n_out, n_in):
    """sel [n_out]: the input index row o picks, (5 o + 3) mod n_in -- not the identity, and onto [0, n_in) once n_out >= n_in (5 is prime to
    every width used here)."""
    assert n_in % 5 != 0
    return (5 * np.arange(n_out) + 3) % n_in


def onehot(n_out, n_in, sel=None):
    """float32 [n_out][n_in] with w[o][sel[o]] = 1 (sel None: the identity, n_out == n_in)."""
    w = np.zeros((n_out, n_in), np.float32)
    w[np.arange(n_out), np.arange(n_out) if sel is None else sel] = 1.0
    return w


# ---- temb bias ----------------------------------------------------------------------------------------------------------------------------
def temb_bias_ref(temb, dw, db, cb):
    out = silu64(temb) @ dw.astype(F64).T + db.astype(F64)
    return out if cb is None else out + cb.astype(F64)


def temb_bias_bound(temb, dw, db, cb):
    """The chain from dense_b, then + conv_b: one more rounding on everything (extra = 1); silu of an exactly given temb."""
    st = silu64(temb)
    base = np.abs(db.astype(F64)) + (0 if cb is None else np.abs(cb.astype(F64)))
    return dot_bound(dw, base, np.abs(st), silu_bound(temb), extra=1)


def temb_bias_f32(temb, dw, db, cb, fused):
    out = row_dot32(dw, silu32(temb), db, fused)
    return out if cb is None else add32(out, cb)


def temb_rows(seed, nt, D):
    """temb [nt][D] float32 ~ 3 N(0, 1), with +-12 planted in every row: where exp(-x) reaches 1.6e5 (the log2e term of the bound matters)
    and where 1 + exp(-x) keeps only 19 bits of exp(-x)."""
    rng = np.random.default_rng(seed)
    x = 3.0 * rng.standard_normal((nt, D))
    x[:, 0], x[:, D - 1] = -12.0, 12.0
    x[:, D // 2] = np.where(np.arange(nt) % 2, 11.7, -11.3)
    return np.clip(x, -12.0, 12.0).astype(np.float32)


def dense_params(seed, D, Cout):
    """dense_w [Cout][D], dense_b [Cout], conv_b [Cout], float32."""
    rng = np.random.default_rng(seed)
    return tuple(np.ascontiguousarray(a, np.float32) for a in (rng.standard_normal((Cout, D)) / np.sqrt(D), 0.3 * rng.standard_normal(Cout),
                                                               0.3 * rng.standard_normal(Cout)))


def job_couts(njobs):
    return [COUTS[j % len(COUTS)] for j in range(njobs)]


# ---- the reference anchor (tests/golden/make_golden_temb.py) ---------------------------------------------------------------------------------
GOLDEN_NFS = (64, 128)
GOLDEN_COUT = 33


def golden_inputs(nf):
    """The seeded inputs of the fixture: t [8], the time-embedding weights (W = 16 N(0, 1)), and one Dense_0 + Conv_0.bias of GOLDEN_COUT rows."""
    t = times(8, np.random.default_rng(1000 + nf))
    return dict(zip(("t", "W", "w1", "b1", "w2", "b2", "dw", "db", "cb"), (t,) + temb_weights(2000 + nf, nf) + dense_params(3000 + nf, 4 * nf, GOLDEN_COUT)))


def checksum(arrays):
    """crc32 over the bytes of the arrays of a dict, in key order."""
    c = 0
    for k in sorted(arrays):
        c = zlib.crc32(np.ascontiguousarray(arrays[k]).tobytes(), c)
    return c


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------
def refusal_cases(lib, p):
    """[(label, call, message)]: one call per argument check of the four entry points (the label's first word is the entry point, which
    the error text must name as well); `p` = any valid, 16-byte aligned, non-null pointer
    (never dereferenced: a refused call launches nothing).  Shared by the CPU test (host memory) and the GPU test (a sentinel buffer)."""
    N = None
    q = C.c_void_p(p.value + 4)                                   # 4-byte aligned only
    imm = C.c_float(0.5)
    big_nf, big_dim = 64 * 1024 // 24 + 2, 64 * 1024 // 4 + 4     # 6 nf floats / temb_dim floats just above 64 KiB
    te = lambda **k: [k.get(a, d) for a, d in (("t", p), ("nt", 1), ("W", p), ("nf", 8), ("w1", p), ("b1", p), ("w2", p), ("b2", p), ("out", p))]
    tb = lambda **k: [k.get(a, d) for a, d in (("temb", p), ("nt", 1), ("D", 32), ("dw", p), ("db", p), ("cb", p), ("Cout", 8), ("out", p))]
    cases = []
    for name, fn in (("fd_time_embedding", lambda a: lib.fd_time_embedding(*a, N)),
                     ("fd_op_time_embedding", lambda a: lib.fd_op_time_embedding(a[0], imm, *a[1:], N))):
        rows = [("W", dict(W=N), "null pointer (gfp_w)"), ("w1", dict(w1=N), "null pointer (w1 / b1)"), ("b1", dict(b1=N), "null pointer (w1 / b1)"),
                ("w2", dict(w2=N), "null pointer (w2 / b2)"), ("b2", dict(b2=N), "null pointer (w2 / b2)"), ("out", dict(out=N), "null pointer (temb)"),
                ("nt 0", dict(nt=0), "nt must be in"), ("nt -1", dict(nt=-1), "nt must be in"), ("nt 2^24", dict(nt=1 << 24), "nt must be in"),
                ("nf 0", dict(nf=0), "nf must be even"), ("nf 1", dict(nf=1), "nf must be even"), ("nf 7", dict(nf=7), "nf must be even"),
                ("nf -2", dict(nf=-2), "nf must be even"), ("nf lds", dict(nf=big_nf), "shared memory"), ("nf 2^30", dict(nf=1 << 30), "shared memory"),
                ("w1 align", dict(w1=q), "w1 is not 16-byte aligned"), ("w2 align", dict(w2=q), "w2 is not 16-byte aligned")]
        if name == "fd_time_embedding":
            rows.append(("t", dict(t=N), "null pointer (t)"))
        cases += [(f"{name} {lab}", (lambda fn=fn, kw=kw: fn(te(**kw))), msg) for lab, kw, msg in rows]
    single = lambda a: lib.fd_temb_bias(a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7], N)

    def jobs(a, njobs=1, tables=True, cb_null_at=None):
        n = max(min(njobs, 4), 1)                                 # the tables are read only once njobs has passed its check
        col = lambda v, hole=None: (C.c_void_p * n)(*[None if (hole is not None and j == hole) else (v.value if v is not None else None) for j in range(n)])
        cout = (C.c_int * n)(*([a[6]] * n))
        if not tables:
            return lib.fd_op_temb_bias_jobs(a[0], a[1], a[2], None, col(a[4]), col(a[5]), col(a[7]), cout, njobs, N)
        return lib.fd_op_temb_bias_jobs(a[0], a[1], a[2], col(a[3]), col(a[4]), col(a[5], cb_null_at), col(a[7]), cout, njobs, N)

    for name, fn in (("fd_temb_bias", single), ("fd_op_temb_bias_jobs", jobs)):
        rows = [("temb", dict(temb=N), "null pointer (temb)"), ("dw", dict(dw=N), "null pointer (dense_w / dense_b"), ("db", dict(db=N), "null pointer (dense_w / dense_b"),
                ("out", dict(out=N), "null pointer (out"), ("nt 0", dict(nt=0), "nt must be in"), ("nt -3", dict(nt=-3), "nt must be in"),
                ("D 0", dict(D=0), "temb_dim must be a multiple of 4"), ("D 2", dict(D=2), "temb_dim must be a multiple of 4"),
                ("D 6", dict(D=6), "temb_dim must be a multiple of 4"), ("D -4", dict(D=-4), "temb_dim must be a multiple of 4"),
                ("D lds", dict(D=big_dim), "shared memory"), ("Cout 0", dict(Cout=0), "must be >= 1"), ("Cout -1", dict(Cout=-1), "must be >= 1"),
                ("dw align", dict(dw=q), "is not 16-byte aligned")]
        cases += [(f"{name} {lab}", (lambda fn=fn, kw=kw: fn(tb(**kw))), msg) for lab, kw, msg in rows]
    cases += [("fd_temb_bias nt 2^24", lambda: single(tb(nt=1 << 24)), "nt must be in"),
              ("fd_op_temb_bias_jobs nt 65536", lambda: jobs(tb(nt=65536)), "nt must be in [1, 65535]"),
              ("fd_op_temb_bias_jobs njobs 0", lambda: jobs(tb(), njobs=0), "njobs must be in"),
              ("fd_op_temb_bias_jobs njobs -1", lambda: jobs(tb(), njobs=-1), "njobs must be in"),
              ("fd_op_temb_bias_jobs njobs 2^24", lambda: jobs(tb(), njobs=1 << 24), "njobs must be in"),
              ("fd_op_temb_bias_jobs tables", lambda: jobs(tb(), tables=False), "null pointer (job tables)"),
              ("fd_op_temb_bias_jobs conv_b", lambda: jobs(tb(cb=N)), "null pointer (conv_b of job 0)"),
              ("fd_op_temb_bias_jobs conv_b of job 2", lambda: jobs(tb(), njobs=3, cb_null_at=2), "null pointer (conv_b of job 2)")]
    return cases


# ---- the cases of the GPU tests, shared with the CPU test (which runs the float32 restatements on exactly these inputs) -----------------
def seed_of(*key):
    return zlib.crc32("/".join(str(k) for k in key).encode())


def embedding_cases():
    """[(label, nf, nt, reach)]: every width x every row count with W = 16 N(0, 1), and two cases whose angles reach 2000 rad."""
    return [(f"nf{nf}_nt{nt}", nf, nt, None) for nf in NFS for nt in NTS] + [(f"nf{nf}_nt3_2000rad", nf, 3, 2000.0) for nf in (24, 128)]


def embedding_inputs(nf, nt, reach=None):
    """-> (t, W, w1, b1, w2, b2)"""
    s = seed_of("emb", nf, nt, reach)
    return (times(nt, np.random.default_rng(s)),) + temb_weights(s + 1, nf, reach)


def bias_cases():
    """[(D, Cout, nt)]: every temb_dim x every Cout at nt = 3; at nt = 1 and 256 each temb_dim and each Cout at least once."""
    ends = ((4, 1), (32, 33), (96, 257), (256, 8), (512, 512), (256, 256))
    return [(D, Cout, 3) for D in TEMB_DIMS for Cout in COUTS] + [(D, Cout, nt) for nt in (1, 256) for D, Cout in ends]


def bias_inputs(D, Cout, nt):
    """-> (temb, dense_w, dense_b, conv_b)"""
    s = seed_of("bias", D, Cout, nt)
    return (temb_rows(s, nt, D),) + dense_params(s + 1, D, Cout)
