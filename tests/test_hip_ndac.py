"""NDAC codec on the GPU (csrc/ndac.hip through the C ABI) against oracle/ndac_oracle.py: operator level (fd_conv1d /
fd_conv_transpose1d with fused Snake / residual / tanh), the residual vector quantiser (code indices BIT-EXACT, ties -> lowest
index), encode / from_codes / decode of the whole codec at a small configuration and at ndac-75's shape (hop 640, 10 x 1024 x 8
codebooks, reduced widths), and the demo.ipynb chain NDAC -> FlowDec.  The oracle restates descript-audio-codec 1.0.0, which is
not available offline: PARITY UNPINNED (see the oracle's header); tests/test_ndac_cpu.py pins the oracle to PyTorch's layers."""
import math

import numpy as np
import pytest
import torch

from conftest import rel_err
from oracle import ndac_oracle as N
from test_hip_ops import check, dev, report
from test_ndac_cpu import NDAC75_LIKE, SMALL, scaled_sd

pytestmark = pytest.mark.gpu


TOL_MFMA_DECODE = 1e-4   # of the waveform peak: split-bf16 operands (3 products, f32 accumulation) + hardware sine in Snake


def lib_call(fn, *a):
    from flowdec_amd import _lib as L
    L.check(getattr(L.load(), fn)(*a))


CONV1D_CASES = [
    # name, B, Ci, T, Co, K, stride, pad, dil, alpha, residual, tanh
    ("first_conv", 2, 1, 300, 8, 7, 1, 3, 1, False, False, False),
    ("res7_dil1", 2, 16, 257, 16, 7, 1, 3, 1, True, False, False),
    ("res7_dil3", 2, 16, 257, 16, 7, 1, 9, 3, True, False, False),
    ("res7_dil9", 1, 24, 200, 24, 7, 1, 27, 9, True, False, False),
    ("res1x1_residual", 2, 16, 130, 16, 1, 1, 0, 1, True, True, False),
    ("down_s2", 2, 8, 256, 16, 4, 2, 1, 1, True, False, False),
    ("down_s8", 1, 40, 1024, 80, 16, 8, 4, 1, True, False, False),
    ("down_s10", 1, 12, 640, 24, 20, 10, 5, 1, True, False, False),
    ("down_s5_ragged", 2, 9, 203, 33, 10, 5, 3, 1, True, False, False),
    ("final_tanh", 2, 12, 500, 1, 7, 1, 3, 1, True, False, True),
    ("latent_k3", 1, 70, 37, 64, 3, 1, 1, 1, True, False, False),
]


@pytest.mark.parametrize("case", CONV1D_CASES, ids=[c[0] for c in CONV1D_CASES])
def test_conv1d(case):
    from flowdec_amd import _lib as L
    name, B, Ci, T, Co, K, s, p, d, use_alpha, use_res, use_tanh = case
    import zlib
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    x = rng.standard_normal((B, Ci, T)).astype(np.float32)
    w = (rng.standard_normal((Co, Ci, K)) / np.sqrt(Ci * K)).astype(np.float32)
    b = rng.standard_normal(Co).astype(np.float32)
    alpha = (1 + 0.3 * rng.standard_normal(Ci)).astype(np.float32) if use_alpha else None
    ref = N.conv1d(N.snake(x, alpha) if use_alpha else x, w, b, stride=s, padding=p, dilation=d)
    res = rng.standard_normal(ref.shape).astype(np.float32) if use_res else None
    if use_res:
        ref = ref + res
    if use_tanh:
        ref = np.tanh(ref)
    out = torch.empty(ref.shape, dtype=torch.float32, device="cuda")
    dx, dw, db, da, dr = dev(x), dev(w), dev(b), dev(alpha) if use_alpha else None, dev(res) if use_res else None   # (kept alive across the launch)
    lib_call("fd_conv1d", L.ptr(dx), L.ptr(dw), L.ptr(db), L.ptr(da), L.ptr(dr), L.ptr(out), B, Ci, T, Co, K, s, p, d, int(use_tanh), L.stream())
    check(f"ndac_conv1d[{name}]", out.cpu().numpy(), ref, 1e-5)


@pytest.mark.parametrize("K,d", [(7, 1), (7, 3), (7, 9), (1, 1), (3, 1)])
def test_conv1d_s1_kernel_bits_equal_generic(K, d):
    """ndac.hip: conv1d_s1_kernel<K, D> (Co >= 4) and the generic conv1d_kernel (Co = 2, 3) accumulate every output in the same fma
    order, so the same weight rows give the same bits -- with the input Snake, a residual, a partial input-channel chunk and a ragged end."""
    from flowdec_amd import _lib as L
    rng = np.random.default_rng(100 * K + d)
    B, Ci, T, Co = 2, 20, 301, 8
    p = (K - 1) * d // 2
    x = rng.standard_normal((B, Ci, T)).astype(np.float32)
    w = (rng.standard_normal((Co, Ci, K)) / np.sqrt(Ci * K)).astype(np.float32)
    b = rng.standard_normal(Co).astype(np.float32)
    alpha = (1 + 0.3 * rng.standard_normal(Ci)).astype(np.float32)
    res = rng.standard_normal((B, Co, T)).astype(np.float32)
    dx, da = dev(x), dev(alpha)

    def conv(rows):
        n = len(rows)
        out = torch.full((B, n, T), float("nan"), device="cuda")
        dw, db, dr = dev(w[rows]), dev(b[rows]), dev(res[:, rows])
        lib_call("fd_conv1d", L.ptr(dx), L.ptr(dw), L.ptr(db), L.ptr(da), L.ptr(dr), L.ptr(out), B, Ci, T, n, K, 1, p, d, 0, L.stream())
        return out.cpu().numpy()

    full = conv(list(range(Co)))                                           # conv1d_s1_kernel<K, d>
    check(f"ndac_conv1d_s1_k{K}_d{d}", full, N.conv1d(N.snake(x, alpha), w, b, padding=p, dilation=d) + res, 1e-5)
    for rows in ([0, 1, 2], [3, 4, 5], [6, 7]):                            # conv1d_kernel (Co < 4)
        assert np.array_equal(conv(rows), full[:, rows]), f"K {K} dilation {d}: rows {rows} differ between the two kernels"


@pytest.mark.parametrize("s,Ci,Co,T", [(2, 16, 8, 100), (4, 24, 12, 77), (8, 48, 24, 40), (10, 20, 10, 33), (5, 9, 7, 50)])
def test_conv_transpose1d(s, Ci, Co, T):
    from flowdec_amd import _lib as L
    rng = np.random.default_rng(s * 1000 + T)
    B, K, p = 2, 2 * s, math.ceil(s / 2)
    x = rng.standard_normal((B, Ci, T)).astype(np.float32)
    w = (rng.standard_normal((Ci, Co, K)) / np.sqrt(Ci * 2)).astype(np.float32)
    b = rng.standard_normal(Co).astype(np.float32)
    alpha = (1 + 0.3 * rng.standard_normal(Ci)).astype(np.float32)
    ref = N.conv_transpose1d(N.snake(x, alpha), w, b, stride=s, padding=p)
    out = torch.empty(ref.shape, dtype=torch.float32, device="cuda")
    dx, dw, db, da = dev(x), dev(w), dev(b), dev(alpha)
    lib_call("fd_conv_transpose1d", L.ptr(dx), L.ptr(dw), L.ptr(db), L.ptr(da), L.ptr(out), B, Ci, T, Co, K, s, p, L.stream())
    check(f"ndac_convtr1d[s={s}]", out.cpu().numpy(), ref, 1e-5)


def build(cfg, seed, gain):
    from flowdec_amd.ndac import DAC
    sd = scaled_sd(cfg, seed, gain)
    m = DAC(**cfg)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return m.cuda(), N.DACOracle(sd, **cfg)


@pytest.mark.parametrize("cfg,gain,nq", [(SMALL, 0.7, 3), (SMALL, 0.7, None), (NDAC75_LIKE, 0.75, 10), (NDAC75_LIKE, 0.75, 4)],
                         ids=["small_nq3", "small_all", "ndac75_nq10", "ndac75_nq4"])
def test_codec_encode_from_codes_decode(cfg, gain, nq):
    """demo.ipynb cell 3: preprocess -> encode(x, n_quantizers=nq) -> quantizer.from_codes(codes) -> decode(zq)."""
    m, o = build(cfg, 3, gain)
    rng = np.random.default_rng(7)
    x = (0.3 * rng.standard_normal((2, 1, 5 * o.hop_length + 123))).astype(np.float32)
    xp = m.preprocess(torch.from_numpy(x).cuda(), cfg["sample_rate"])
    assert xp.shape[-1] == math.ceil(x.shape[-1] / o.hop_length) * o.hop_length and np.array_equal(xp.cpu().numpy(), o.preprocess(x))
    z, codes, lat, l1, l2 = m.encode(xp, n_quantizers=nq)
    z_o, codes_o, lat_o, _, _ = o.encode(o.preprocess(x), n_quantizers=nq)
    assert l1 is None and l2 is None and codes.dtype == torch.int64 and tuple(codes.shape) == codes_o.shape
    # the encoder output feeding the quantiser agrees to float32 rounding; the quantiser's own arithmetic is reproduced exactly, so the
    # codes can only differ where the two ENCODER outputs round a near-tie differently: compare through the oracle's quantiser on the
    # GPU encoder's latents as well (bit-exact), and directly (exact on this data)
    nqq = codes.shape[1]
    mism = int((codes.cpu().numpy() != codes_o).sum())
    report(f"ndac_codes_mismatch[{nqq}]", float(mism), 0.5)
    assert mism == 0, f"{mism} of {codes_o.size} code indices differ from the oracle"
    check(f"ndac_encode_z[{nqq}]", z.cpu().numpy(), z_o, 2e-5)
    check(f"ndac_encode_latents[{nqq}]", lat.cpu().numpy(), lat_o, 2e-5)
    zq, zp, c2 = m.quantizer.from_codes(codes)
    zq_o, zp_o, _ = o.from_codes(codes_o)
    assert torch.equal(c2, codes)
    check(f"ndac_from_codes[{nqq}]", zq.cpu().numpy(), zq_o, 1e-6)
    assert np.array_equal(zp.cpu().numpy(), zp_o)
    y = m.decode(zq)
    y_o = o.decode(zq_o)
    assert tuple(y.shape) == y_o.shape and float(y.abs().max()) <= 1.0
    check(f"ndac_decode[{nqq}]", y.cpu().numpy(), y_o, TOL_MFMA_DECODE)   # default: the layers ndac_mfma.hip supports run on the matrix cores
    m.precision = "exact"
    check(f"ndac_decode_exact[{nqq}]", m.decode(zq).cpu().numpy(), y_o, 2e-5)
    m.precision = "mfma_decoder"
    out = m(torch.from_numpy(x).cuda(), cfg["sample_rate"], n_quantizers=nq)         # dac.DAC.forward: trimmed to the input length
    assert out["audio"].shape == (2, 1, x.shape[-1]) and torch.equal(out["codes"], codes)


def test_rvq_standalone_bit_exact_and_ties():
    """fd_rvq_encode on a given latent: indices BIT-EXACT against the oracle's float32 operation order on 4096 vectors per codebook,
    duplicated codebook rows (exact ties) resolve to the lowest index, z_q / latents equal to rounding."""
    cfg = dict(NDAC75_LIKE, n_codebooks=6)
    sd = scaled_sd(cfg, 11, 0.75)
    for q in range(cfg["n_codebooks"]):    # exact duplicates at higher indices than the original row
        cb = sd[f"quantizer.quantizers.{q}.codebook.weight"]
        cb[900:932] = cb[100:132]; cb[1000] = cb[3]
    from flowdec_amd.ndac import DAC
    m = DAC(**cfg); m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}); m = m.cuda()
    o = N.DACOracle(sd, **cfg)
    rng = np.random.default_rng(5)
    z = rng.standard_normal((4, o.cfg["latent_dim"], 1024)).astype(np.float32)
    zq, codes, lat, _, _ = m.quantizer(torch.from_numpy(z).cuda(), n_quantizers=6)
    zq_o, codes_o, lat_o = o.quantize(z, 6)
    assert np.array_equal(codes.cpu().numpy(), codes_o), int((codes.cpu().numpy() != codes_o).sum())
    assert not np.isin(codes_o, np.r_[900:932, 1000]).any() and np.isin(codes_o, np.r_[100:132, 3]).any()     # ties went to the lower copy
    check("ndac_rvq_zq", zq.cpu().numpy(), zq_o, 1e-6)
    check("ndac_rvq_latents", lat.cpu().numpy(), lat_o, 1e-6)
    one = m.quantizer(torch.from_numpy(z[1:2, :, 100:164].copy()).cuda(), n_quantizers=6)[1]          # per (b, t): independent of batch / length
    assert torch.equal(one, codes[1:2, :, 100:164])


def test_demo_chain_ndac_into_flowdec():
    """demo.ipynb cells 2-3 end to end on the GPU: NDAC encode / from_codes / decode -> FlowModel.enhance(xhat_ndac)."""
    import flowdec_amd
    from oracle import flowdec_oracle as O
    m, _ = build(NDAC75_LIKE, 3, 0.75)
    fm = flowdec_amd.from_preset("flowdec_75m", precision="bf16", nf=8)
    fm.load_state_dict({k: torch.from_numpy(v) for k, v in O.random_state_dict(seed=8, nf=8).items()}, strict=False)
    fm = fm.cuda()
    g = torch.Generator(device="cuda").manual_seed(0)
    sig = 0.2 * torch.randn(1, 1, 30000, device="cuda", generator=g)
    x = m.preprocess(sig, 48000)
    z, codes, latents, _, _ = m.encode(x, n_quantizers=10)
    zq, _, _ = m.quantizer.from_codes(codes)
    xhat_ndac = m.decode(zq)
    assert xhat_ndac.shape == (1, 1, x.shape[-1]) and torch.isfinite(xhat_ndac).all()
    xhat = fm.enhance(xhat_ndac, N=3, solver="midpoint", generator=g)
    assert xhat.shape == xhat_ndac.shape and torch.isfinite(xhat).all() and xhat.is_cuda


# decoder wide enough for csrc/ndac_mfma.hip: 768 -> 384 (x10) -> 192 (x8) -> 96 (x4) on the matrix cores (96-channel tiles, transposed
# convolutions as stride phases), 96 -> 48 (x2) and the final 48 -> 1 convolution on the exact vector path (mixed walk)
WIDE_DECODER = dict(NDAC75_LIKE, decoder_dim=768, n_codebooks=4)


@pytest.mark.parametrize("cfg,frames,batch", [(WIDE_DECODER, 7, 2), (WIDE_DECODER, 1, 1), (dict(SMALL, decoder_dim=256), 53, 3)],
                         ids=["wide_7f", "wide_1f", "small256_53f"])
def test_decoder_on_matrix_cores(cfg, frames, batch):
    """dac.DAC.decode with the decoder's convolutions on MFMA (the default) against the oracle and against the exact vector path."""
    from flowdec_amd import _lib as L
    m, o = build(cfg, 5, 0.6)   # (gain: output peak ~0.5, tanh unsaturated)
    rng = np.random.default_rng(frames)
    codes = rng.integers(0, cfg["codebook_size"], size=(batch, cfg["n_codebooks"], frames))
    zq_o, _, _ = o.from_codes(codes)
    zq = m.quantizer.from_codes(torch.from_numpy(codes).cuda())[0]
    assert m.precision == "mfma_decoder"
    y = m.decode(zq)
    assert L.load().fd_ndac_get_precision(m.handle()) == 1
    y_o = o.decode(zq_o)
    assert tuple(y.shape) == y_o.shape
    check(f"ndac_decode_mfma[{frames}x{batch}]", y.cpu().numpy(), y_o, TOL_MFMA_DECODE)
    m.precision = "exact"
    y_e = m.decode(zq)
    assert L.load().fd_ndac_get_precision(m.handle()) == 0
    check(f"ndac_decode_exact[{frames}x{batch}]", y_e.cpu().numpy(), y_o, 2e-5)
    assert not torch.equal(y, y_e), "the two precisions returned identical bits: the matrix-core path did not run"
    m.precision = "bf16"
    with pytest.raises(ValueError):
        m.decode(zq)


WIDE_ENCODER = dict(NDAC75_LIKE, encoder_dim=32, n_codebooks=4)     # 32 -> 64 (/2) -> 128 (/4) -> 256 (/8) -> 512 (/10): strides 2, 4, 8, 10 on MFMA
WIDE_ENCODER_S5 = dict(SMALL, encoder_dim=32)                       # 32 -> 64 (/2) -> 128 (/4) -> 256 (/5): the odd stride (16-bit LDS writes)


@pytest.mark.parametrize("cfg,hops,batch", [(WIDE_ENCODER, 5, 2), (WIDE_ENCODER, 1, 1), (WIDE_ENCODER_S5, 41, 3)], ids=["wide_5h", "wide_1h", "s5_41h"])
def test_encoder_on_matrix_cores(cfg, hops, batch):
    """precision="mfma": the encoder's convolutions (strided ones in polyphase form) on the matrix cores.  The latent entering the
    quantiser agrees with the oracle to TOL_MFMA_DECODE; code indices may differ from the exact path only at near-ties."""
    m, o = build(cfg, 9, 0.7)
    rng = np.random.default_rng(hops)
    x = (0.3 * rng.standard_normal((batch, 1, hops * o.hop_length))).astype(np.float32)
    xd = torch.from_numpy(x).cuda()
    m.precision = "mfma"
    z, codes, lat, _, _ = m.encode(xd)
    m.precision = "exact"
    z_e, codes_e, lat_e, _, _ = m.encode(xd)
    z_o, codes_o, lat_o, _, _ = o.encode(x)
    assert np.array_equal(codes_e.cpu().numpy(), codes_o)
    cd = cfg["codebook_dim"]
    check(f"ndac_encode_mfma_latent0[{hops}x{batch}]", lat[:, :cd].cpu().numpy(), lat_o[:, :cd], TOL_MFMA_DECODE)   # in_proj_0(encoder(x)): no quantiser decision in it
    assert not torch.equal(lat[:, :cd], lat_e[:, :cd]), "identical bits: the matrix-core path did not run"
    frac = float((codes != codes_e).float().mean())
    report(f"ndac_encode_mfma_code_mismatch_fraction[{hops}x{batch}]", frac, 0.02)
    assert frac <= 0.02, f"{frac:.4f} of the code indices differ from the exact path"
    same = (codes == codes_e).all(dim=1, keepdim=True).expand(-1, z.shape[1], -1)    # frames whose whole code stack agrees: same z_q up to rounding
    if bool(same.any()):
        assert float((z - z_e)[same].abs().max()) <= 1e-4 * float(z_e.abs().max())


FULL_WIDTH = dict(encoder_dim=64, encoder_rates=(2, 4, 8, 10), decoder_dim=1536, decoder_rates=(10, 8, 4, 2), n_codebooks=10, codebook_size=1024,
                  codebook_dim=8, sample_rate=48000)   # DAC's published widths at ndac-75's frame rate: what scripts/ndac_bench.py times


def test_codec_full_width_three_frames():
    """Every layer shape of the full-width codec (1536 ... 96 decoder channels, 64 ... 1024 encoder channels, strides 2 / 4 / 8 / 10 both
    ways) on three frames: exact encode (code indices = oracle), matrix-core decode and exact decode against the oracle, matrix-core
    encode against the exact one."""
    m, o = build(FULL_WIDTH, 5, 0.55)
    rng = np.random.default_rng(11)
    x = (0.3 * rng.standard_normal((1, 1, 3 * o.hop_length))).astype(np.float32)
    xd = torch.from_numpy(x).cuda()
    z, codes, lat, _, _ = m.encode(xd)
    z_o, codes_o, lat_o, _, _ = o.encode(x)
    assert np.array_equal(codes.cpu().numpy(), codes_o)
    check("ndac_full_encode_latents", lat.cpu().numpy(), lat_o, 2e-5)
    zq = m.quantizer.from_codes(codes)[0]
    y_o = o.decode(o.from_codes(codes_o)[0])
    assert float(np.abs(y_o).max()) < 0.999   # (tanh not saturated: the comparison sees the decoder)
    check("ndac_full_decode_mfma", m.decode(zq).cpu().numpy(), y_o, TOL_MFMA_DECODE)
    m.precision = "exact"
    check("ndac_full_decode_exact", m.decode(zq).cpu().numpy(), y_o, 2e-5)
    m.precision = "mfma"
    _, codes_m, lat_m, _, _ = m.encode(xd)
    cd = FULL_WIDTH["codebook_dim"]
    check("ndac_full_encode_mfma_latent0", lat_m[:, :cd].cpu().numpy(), lat_o[:, :cd], TOL_MFMA_DECODE)
    assert float((codes_m != codes).float().mean()) <= 0.1   # 30 indices: at most 3 near-ties


def test_codec_full_size_batch_independence():
    """BASELINE-sized codec calls (full width, 8 x 2 s) through properties that need no oracle: a clip gives the same bits alone and in
    the batch (the matrix-core kernels pick 128- or 256-position workgroups by the GRID size, the K order per output is the same), for
    encode (exact path: codes, latents), from_codes and decode (matrix cores and exact); decode(from_codes(encode(x))) is finite, inside
    (-1, 1) and as long as the input."""
    from flowdec_amd.ndac import DAC
    torch.manual_seed(0)
    m = DAC(**FULL_WIDTH)
    for k, p in m.named_parameters():          # keep activations O(1): g = 0.8 ||v||
        if k.endswith("weight_g"):
            v = dict(m.named_parameters())[k[:-1] + "v"]
            p.data = 0.8 * v.data.pow(2).sum(dim=tuple(range(1, v.ndim)), keepdim=True).sqrt()
    m = m.cuda()
    x = m.preprocess(0.3 * torch.randn(8, 1, 96000, device="cuda"), 48000)
    z, codes, lat, _, _ = m.encode(x)
    zq = m.quantizer.from_codes(codes)[0]
    y = m.decode(zq)
    assert y.shape == x.shape and torch.isfinite(y).all() and float(y.abs().max()) <= 1.0
    for b in (0, 5):
        z1, c1, l1, _, _ = m.encode(x[b:b + 1])
        assert torch.equal(c1[0], codes[b]) and torch.equal(l1[0], lat[b]) and torch.equal(z1[0], z[b])
        assert torch.equal(m.quantizer.from_codes(codes[b:b + 1])[0][0], zq[b])
        assert torch.equal(m.decode(zq[b:b + 1])[0], y[b])
    m.precision = "exact"
    ye = m.decode(zq)
    assert torch.equal(m.decode(zq[3:4])[0], ye[3])
    assert float((y - ye).abs().max()) <= TOL_MFMA_DECODE * float(ye.abs().max())
    m.precision = "mfma"
    zm, cm, lm, _, _ = m.encode(x)
    z1, c1, l1, _, _ = m.encode(x[2:3])
    assert torch.equal(c1[0], cm[2]) and torch.equal(l1[0], lm[2])
    assert float((cm != codes).float().mean()) <= 0.02
