"""CPU-only checks of the host side of csrc/ndac_mfma.hip (the codec's matrix-core convolution): the packed A-operand layout against
a NumPy mirror of the layout documented above fd_ndac_mfma_pack, the hi / lo split, the launch-variant rule against a Python mirror of
fd_ndac_mfma_supported + block_mt + the NT rule, and the host-side refusals.  The GPU side is tests/test_hip_ndac_mfma.py."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

CK, TN, ROWB = 32, 256, 80
FD_EINVAL = -1


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from flowdec_amd import _lib
    return _lib.load()


def bf16_rne(v):
    """float32 -> bf16 bits, round to nearest even (finite inputs)."""
    u = np.ascontiguousarray(v, np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def bf16_f32(h):
    return (h.astype(np.uint32) << 16).view(np.float32)


def block_mt(Co):
    return 3 if Co % 96 == 0 else (2 if Co % 64 == 0 else 0)


def supported(Ci, Co, K, stride, dil, tr):
    if Ci <= 0 or not block_mt(Co) or K <= 0 or stride <= 0 or dil <= 0:
        return False
    if not tr and stride > 1:
        if stride not in (2, 4, 5, 8, 10) or K % stride or dil != 1:
            return False
    else:
        if Ci % CK:
            return False
        if (K % stride or dil != 1) if tr else stride != 1:
            return False
    span = K // stride - 1 if stride > 1 else (K - 1) * dil
    return (TN + span) * ROWB * 2 <= 64 * 1024


def variant(B, Ci, T, Co, K, stride, pad, dil, tr):
    """(MT, S, NT, grid.x, grid.y) of the launch, or None where the host refuses the shape."""
    if B <= 0 or T <= 0 or pad < 0 or not supported(Ci, Co, K, stride, dil, tr):
        return None
    if tr:
        ntaps, nphase, S = K // stride, stride, 0
        To, N = (T - 1) * stride - 2 * pad + K, T + K // stride - 1
    elif stride > 1:
        ntaps, nphase, S = K // stride, 1, stride
        To = (T + 2 * pad - K) // stride + 1
        N = To
    else:
        ntaps, nphase, S = K, 1, 0
        To = T + 2 * pad - dil * (K - 1)
        N = To
    if To <= 0:
        return None
    mt = block_mt(Co)
    ncob = Co // (32 * mt)
    wgs256 = -(-N // TN) * ncob * nphase * B
    nt = 2 if wgs256 >= 512 else 1
    return (mt, S, nt, -(-N // (128 * nt)), ncob * nphase)


def want_values(w, Ci, Co, K, stride, tr):
    """The float32 weight at each position of the layout documented above fd_ndac_mfma_pack, from the PyTorch weight ([Co][Ci][K], or
    [Ci][Co][K] if transposed): [phase * Co / CB + co block][chunk][tap][16-element block][32-co tile][lane][8] (0 where no weight)."""
    wc = np.transpose(w, (0, 2, 1)) if tr else np.transpose(w, (1, 2, 0))        # -> [Ci][K][Co]
    mt_n = block_mt(Co)
    CB, ncob = 32 * mt_n, Co // (32 * mt_n)
    strided = not tr and stride > 1
    nphase, ntaps = (stride if tr else 1), (K // stride if stride > 1 else K)
    cpc = CK // stride if strided else CK
    nchunk = -(-Ci // cpc) if strided else Ci // CK
    ph, cob, chunk, tap, kb, mt, lane, j = np.ix_(*[np.arange(n) for n in (nphase, ncob, nchunk, ntaps, 2, mt_n, 64, 8)])
    co = cob * CB + 32 * mt + (lane & 31)
    e = kb * 16 + (lane >> 5) * 8 + j
    if strided:
        ci = chunk * cpc + e // stride
        k = e % stride + tap * stride
        valid = (e < cpc * stride) & (ci < Ci)
    else:
        ci = chunk * CK + e
        k = ph + tap * stride if tr else tap + 0 * ph
        valid = np.ones(ci.shape, bool)
    ci, k, co, valid = np.broadcast_arrays(ci, k, co, valid)
    return np.where(valid, wc[np.minimum(ci, Ci - 1), k, co], np.float32(0))


def pack_mirror(w, Ci, Co, K, stride, tr):
    """The packed uint16 buffer: [...][32-co tile][hi | lo][lane][8] bf16 bits, then one step of zeros (the kernel's last prefetch)."""
    v = want_values(w, Ci, Co, K, stride, tr)
    hi = bf16_rne(v)
    lo = bf16_rne(v - bf16_f32(hi))
    out = np.stack([hi, lo], axis=6)       # [ph][cob][chunk][tap][kb][mt][hi|lo][lane][8]
    return np.concatenate([out.ravel(), np.zeros(3 * 2 * 64 * 8, np.uint16)])


PACK_CASES = [  # Ci, Co, K, stride, transposed
    (32, 96, 7, 1, False), (64, 64, 1, 1, False), (96, 192, 3, 1, False), (32, 128, 7, 1, False),
    (32, 96, 4, 2, True), (64, 64, 8, 4, True), (32, 96, 10, 5, True), (32, 128, 16, 8, True), (64, 192, 20, 10, True),
    (17, 64, 4, 2, False), (9, 96, 8, 4, False), (40, 96, 10, 5, False), (5, 128, 16, 8, False), (40, 192, 20, 10, False),
    (3, 64, 20, 10, False), (6, 96, 10, 5, False),
]


@pytest.mark.parametrize("Ci,Co,K,stride,tr", PACK_CASES, ids=["Ci%d_Co%d_K%d_s%d%s" % (c[0], c[1], c[2], c[3], "T" if c[4] else "") for c in PACK_CASES])
def test_pack_matches_layout_mirror(lib, Ci, Co, K, stride, tr):
    from flowdec_amd import ops
    rng = np.random.default_rng(Ci * 1000 + Co + K)
    w = (rng.standard_normal((Ci, Co, K) if tr else (Co, Ci, K)) * np.exp2(rng.integers(-12, 4, (Ci, Co, K) if tr else (Co, Ci, K)))).astype(np.float32)
    got = ops.ndac_mfma_pack_weights(w, stride, tr)
    want = pack_mirror(w, Ci, Co, K, stride, tr)
    assert lib.fd_ndac_mfma_packed_bytes(Ci, Co, K, stride, int(tr)) == 2 * want.size
    assert got.shape == want.shape and np.array_equal(got, want), f"{int((got != want).sum())} of {want.size} packed halfwords differ"
    assert not got[-3 * 2 * 64 * 8:].any()                           # the prefetch padding step is there and zero
    # hi + lo reconstructs every weight to 2^-16 relative (the test below pins the rounding itself), and every weight is used once
    hi, lo = got[:-3 * 2 * 64 * 8].reshape(-1, 2, 512).transpose(1, 0, 2).reshape(2, -1)
    rec = bf16_f32(hi).astype(np.float64) + bf16_f32(lo).astype(np.float64)
    v = want_values(w, Ci, Co, K, stride, tr).ravel().astype(np.float64)
    assert np.all(np.abs(rec - v) <= 2.0 ** -16 * np.abs(v))
    assert np.array_equal(np.sort(np.abs(v[v != 0])), np.sort(np.abs(w[w != 0].astype(np.float64))))


def test_split_is_round_to_nearest_even(lib):
    """hi is torch's RNE bf16 rounding of w (ties included), lo the RNE rounding of the remainder, |w - hi - lo| <= 2^-16 |w|."""
    from flowdec_amd import ops
    rng = np.random.default_rng(3)
    Ci, Co, K = 32, 64, 1
    w = (rng.standard_normal((Co, Ci, K)) * np.exp2(rng.integers(-20, 20, (Co, Ci, K)))).astype(np.float32)
    w.ravel()[:64] = bf16_f32(np.arange(0x3F80, 0x3FC0, dtype=np.uint16)) + np.float32(2.0 ** -8)   # exact ties: 1.x + half a bf16 ulp
    got = ops.ndac_mfma_pack_weights(w).reshape(-1)[:-3 * 2 * 64 * 8].reshape(2, 2, 1, 2, 64, 8)   # [kb][mt][.][hi|lo][lane][8]
    # lane l, element j of block kb: co = 32 mt + (l & 31), ci = 16 kb + 8 (l >> 5) + j
    kb, mt, lane, j = np.ix_(np.arange(2), np.arange(2), np.arange(64), np.arange(8))
    co, ci = 32 * mt + (lane & 31), 16 * kb + 8 * (lane >> 5) + j
    wv = w[co, ci, 0]
    hi, lo = got[:, :, 0, 0], got[:, :, 0, 1]
    t_hi = torch.from_numpy(wv.copy()).to(torch.bfloat16)
    assert np.array_equal(hi, t_hi.view(torch.int16).numpy().view(np.uint16))
    t_lo = (torch.from_numpy(wv.copy()) - t_hi.float()).to(torch.bfloat16)
    assert np.array_equal(lo, t_lo.view(torch.int16).numpy().view(np.uint16))
    rec = bf16_f32(hi).astype(np.float64) + bf16_f32(lo).astype(np.float64)
    assert np.all(np.abs(rec - wv) <= 2.0 ** -16 * np.abs(wv))


def variant_sweep():
    cases = []
    for Co in (32, 48, 64, 96, 128, 160, 192, 256, 384, 768, 1536):
        cases += [(1, 32, 300, Co, 7, 1, 3, 1, False), (2, 64, 100, Co, 4, 2, 1, 1, True), (1, 17, 999, Co, 10, 5, 3, 1, False)]
    for K, d in ((7, 1), (7, 3), (7, 9), (7, 40), (7, 41), (7, 42), (7, 43), (3, 1), (1, 1), (3, 5), (2, 151), (155, 1), (154, 1), (153, 1)):
        for Ci in (32, 40, 1536, 48):
            cases.append((2, Ci, 5000, 96, K, 1, (K - 1) * d // 2, d, False))
    for s in (1, 2, 3, 4, 5, 6, 8, 10, 16):
        for K in (2 * s, 3 * s, 2 * s + 1, s, 200):
            cases += [(3, 64, 77, 192, K, s, (s + 1) // 2, 1, True), (3, 33, 3000, 192, K, s, (s + 1) // 2, 1, False),
                      (3, 33, 3000, 192, K, s, 0, 2, False)]
    for B in (1, 2, 31, 32, 33, 64, 255, 256, 257, 512, 513):      # the NT threshold: wgs256 >= 512
        cases += [(B, 32, 700, 96, 7, 1, 3, 1, False), (B, 32, 511, 128, 3, 1, 1, 1, False), (B, 32, 257, 192, 1, 1, 0, 1, False),
                  (B, 96, 50, 96, 4, 2, 1, 1, True), (B, 96, 31, 384, 20, 10, 5, 1, True), (B, 7, 2570, 64, 20, 10, 5, 1, False)]
    for Co in (96, 128):                                           # every (MT, S, NT) instantiation
        for s in (2, 4, 5, 8, 10):
            cases += [(B, 7, 300 * s, Co, 2 * s, s, (s + 1) // 2, 1, False) for B in (1, 600)]
        cases += [(B, 64, 300, Co, 7, 1, 3, 1, False) for B in (1, 600)]
    cases += [(1, 32, 1, 96, 20, 10, 5, 1, True), (1, 32, 2, 96, 8, 4, 2, 1, True), (1, 32, 3, 96, 7, 1, 0, 1, False),
              (1, 32, 6, 96, 7, 1, 0, 1, False), (1, 32, 7, 96, 7, 1, 0, 1, False), (0, 32, 100, 96, 7, 1, 3, 1, False),
              (1, 32, 0, 96, 7, 1, 3, 1, False), (1, 32, 100, 96, 7, 1, -1, 1, False), (1, 5, 19, 96, 20, 10, 0, 1, False),
              (1, 5, 20, 96, 20, 10, 0, 1, False), (1, 0, 100, 96, 7, 1, 3, 1, False), (1, 32, 100, 96, 0, 1, 0, 1, False),
              (1, 32, 100, 96, 7, 0, 3, 1, False), (1, 32, 100, 96, 7, 1, 3, 0, False)]
    return cases


def test_variant_rule_matches_mirror(lib):
    from flowdec_amd import ops
    seen = set()
    for c in variant_sweep():
        want = variant(*c)
        v = (C.c_int * 5)(-7, -7, -7, -7, -7)
        rc = lib.fd_ndac_mfma_variant(*c, C.byref(v))
        if want is None:
            assert rc == FD_EINVAL and lib.fd_last_error(), c
            assert list(v) == [-7] * 5, c                                # nothing written on refusal
            continue
        assert rc == 0 and tuple(v) == want, (c, tuple(v), want)
        assert ops.ndac_mfma_variant(*c[:5], stride=c[5], pad=c[6], dil=c[7], transposed=c[8]) == dict(MT=want[0], S=want[1], NT=want[2], grid=want[3:])
        seen.add(want[:3])
        # the packed size is the layout's: nonzero exactly when the (dilation-free) shape is supported
        assert lib.fd_ndac_mfma_packed_bytes(c[1], c[3], c[4], c[5], int(c[8])) > 0
    assert {(mt, s, nt) for mt in (2, 3) for s in (0, 2, 4, 5, 8, 10) for nt in (1, 2)} <= seen
    # the LDS limit: (256 + span) 160 B <= 64 KiB, i.e. span <= 153 -- K = 7 at dilation 25 fits, 26 does not
    assert variant(1, 32, 1000, 96, 7, 1, 0, 25, False) and not variant(1, 32, 1000, 96, 7, 1, 0, 26, False)
    assert lib.fd_ndac_mfma_packed_bytes(32, 80, 7, 1, 0) == 0 and lib.fd_ndac_mfma_packed_bytes(40, 96, 7, 1, 0) == 0


def test_pack_weights_refuses_unsupported(lib):
    w = np.zeros(40 * 96 * 7, np.float32)
    dst = np.zeros(1 << 16, np.uint16)
    for Ci, Co, K, s, tr in ((40, 96, 7, 1, 0), (32, 80, 7, 1, 0), (32, 96, 7, 3, 0), (32, 96, 7, 2, 1), (32, 96, 9, 2, 0)):
        assert lib.fd_ndac_mfma_pack_weights(w.ctypes.data, Ci, Co, K, s, tr, dst.ctypes.data) == FD_EINVAL
        assert b"unsupported" in lib.fd_last_error()
    assert not dst.any()


REFUSALS = r"""
import ctypes as C, sys
sys.path.insert(0, sys.argv[1])
from flowdec_amd import _lib
lib = _lib.load()
p = C.c_void_p(4096)    # never dereferenced: every call below must be refused on the host before any launch
calls = [  # x, packed, bias, residual, out, out_act, alpha_out, B, Ci, T, Co, K, stride, pad, dil, transposed
    ("residual needs the activated output", (p, p, p, p, p, None, None, 1, 32, 64, 96, 7, 1, 3, 1, 0)),
    ("residual needs the activated output", (p, p, p, p, p, None, p, 2, 32, 64, 192, 4, 2, 1, 1, 1)),
    ("residual needs the activated output", (p, p, p, p, p, None, None, 2, 7, 640, 128, 20, 10, 5, 1, 0)),
    ("null argument", (p, p, p, None, None, None, None, 1, 32, 64, 96, 7, 1, 3, 1, 0)),
    ("null argument", (p, p, p, None, None, p, None, 1, 32, 64, 96, 7, 1, 3, 1, 0)),
    ("null argument", (None, p, p, None, p, None, None, 1, 32, 64, 96, 7, 1, 3, 1, 0)),
    ("unsupported", (p, p, p, None, p, None, None, 1, 40, 64, 96, 7, 1, 3, 1, 0)),
    ("unsupported", (p, p, p, None, p, None, None, 1, 32, 64, 80, 7, 1, 3, 1, 0)),
    ("unsupported", (p, p, p, None, p, None, None, 1, 32, 64, 96, 7, 3, 3, 1, 0)),
    ("unsupported", (p, p, p, None, p, None, None, 1, 32, 64, 96, 7, 1, 3, 26, 0)),
    ("unsupported", (p, p, p, None, p, None, None, 1, 32, 64, 96, 9, 2, 1, 1, 1)),
    ("empty output", (p, p, p, None, p, None, None, 1, 32, 5, 96, 7, 1, 0, 1, 0)),
    ("bad shape", (p, p, p, None, p, None, None, 0, 32, 64, 96, 7, 1, 3, 1, 0)),
]
for want, args in calls:
    rc = lib.fd_ndac_mfma_conv1d(*args, None)
    msg = (lib.fd_last_error() or b"").decode()
    assert rc == -1 and want in msg, (want, rc, msg)
print("REFUSED", len(calls))
"""


def test_conv1d_refusals_happen_on_the_host():
    """fd_ndac_mfma_conv1d refuses bad calls with FD_EINVAL before any launch -- among them a residual without out_act, which
    every residual epilogue would store through.  The calls run in a child process that sees no GPU, so a refusal that went
    missing shows as a launch error, never as a launch."""
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1")
    r = subprocess.run([sys.executable, "-c", REFUSALS, ROOT], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "REFUSED 13" in r.stdout, r.stdout + r.stderr
