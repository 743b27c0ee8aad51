"""The residual vector quantiser as ONE launch (csrc/ndac.hip rvq_chain_kernel through fd_rvq_encode_chain) against the chain of
rvq_step_kernel launches (fd_rvq_encode) on the same latent: code indices, z_q and latents BIT-equal -- dense, with a tail tile, on a
single frame, with a prefix of the quantisers, with and without the latents output, on duplicated codebook rows (exact ties), and
under a per-clip frame table, where nothing behind a clip is read and everything behind it comes back as 0.  fd_rvq_encode itself is
pinned to the oracle by tests/test_hip_ndac.py.  Widths: 64 (SMALL, J = 32), 128 (NDAC75_LIKE), 512 (WIDE_ENCODER) and DAC's full
1024 -- the whole LDS budget of the kernel -- on an otherwise small codec."""
import numpy as np
import pytest
import torch

from test_hip_ndac import WIDE_ENCODER, build
from test_ndac_cpu import NDAC75_LIKE, SMALL, scaled_sd

pytestmark = pytest.mark.gpu

CFGS = {"ndac75": NDAC75_LIKE, "wide": WIDE_ENCODER, "small": SMALL, "latent1024": dict(NDAC75_LIKE, latent_dim=1024, n_codebooks=3)}
_models = {}


def model(name):
    if name not in _models:
        _models[name] = build(CFGS[name], 5, 0.6)[0]
    return _models[name]


def latent(m, B, T, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, m.latent_dim, T, generator=g).cuda()


def nq_of(m, n_quantizers):
    return m.n_codebooks if n_quantizers is None else min(n_quantizers, m.n_codebooks)


def run_steps(m, z, n_quantizers, with_latents=True):
    """fd_rvq_encode: one rvq_step_kernel launch per quantiser -> (z_q, codes int32, latents or None)."""
    from flowdec_amd import _lib as L
    B, D, T = z.shape
    nq = nq_of(m, n_quantizers)
    zq = torch.full_like(z, float("nan"))
    codes = torch.full((B, nq, T), -7, dtype=torch.int32, device="cuda")
    lat = torch.full((B, nq * m.codebook_dim, T), float("nan"), device="cuda") if with_latents else None
    ws = torch.empty(z.numel() * 4, dtype=torch.uint8, device="cuda")
    L.check(L.load().fd_rvq_encode(m.handle(), L.ptr(z), B, T, nq, L.ptr(zq), L.ptr(codes), L.ptr(lat), L.ptr(ws), ws.numel(), L.stream()))
    return zq, codes, lat


def run_chain(m, z, n_quantizers, frames=None, with_latents=True):
    """fd_rvq_encode_chain on outputs pre-filled with NaN / -7: everything it is to write, it writes."""
    from flowdec_amd import _lib as L
    B, D, T = z.shape
    nq = nq_of(m, n_quantizers)
    zq = torch.full_like(z, float("nan"))
    codes = torch.full((B, nq, T), -7, dtype=torch.int32, device="cuda")
    lat = torch.full((B, nq * m.codebook_dim, T), float("nan"), device="cuda") if with_latents else None
    fr = None if frames is None else torch.tensor(frames, dtype=torch.int32, device="cuda")
    zin = z.clone()
    L.check(L.load().fd_rvq_encode_chain(m.handle(), L.ptr(zin), L.ptr(fr), B, T, nq, L.ptr(zq), L.ptr(codes), L.ptr(lat), L.stream()))
    assert torch.equal(zin.view(torch.int32), z.view(torch.int32))      # z is read-only
    return zq, codes, lat


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32)) if a.dtype == torch.float32 else torch.equal(a, b)


def test_the_rule_knows_these_widths():
    from flowdec_amd import _lib as L
    lib = L.load()
    assert all(lib.fd_rvq_chain_supported(model(n).latent_dim, 8) == 1 for n in CFGS) and lib.fd_rvq_chain_supported(1056, 8) == 0
    assert [model(n).latent_dim for n in ("small", "ndac75", "wide", "latent1024")] == [64, 128, 512, 1024]


@pytest.mark.parametrize("with_latents", [True, False], ids=["latents", "nolatents"])
@pytest.mark.parametrize("n_quantizers", [None, 3], ids=["all", "nq3"])
@pytest.mark.parametrize("T", [23, 1])
@pytest.mark.parametrize("name", list(CFGS))
def test_chain_equals_the_step_launches(name, T, n_quantizers, with_latents):
    m = model(name)
    z = latent(m, 3, T, 11 + T)
    zq_s, codes_s, lat_s = run_steps(m, z, n_quantizers, with_latents)
    zq_c, codes_c, lat_c = run_chain(m, z, n_quantizers, None, with_latents)
    assert int(codes_s.min()) >= 0 and int(codes_s.max()) < m.codebook_size
    assert torch.equal(codes_c, codes_s), f"{int((codes_c != codes_s).sum())} of {codes_s.numel()} code indices differ from the step launches"
    assert same_bits(zq_c, zq_s), f"{int((zq_c.view(torch.int32) != zq_s.view(torch.int32)).sum())} of {zq_s.numel()} z_q values differ in their bits"
    if with_latents:
        assert same_bits(lat_c, lat_s), f"{int((lat_c.view(torch.int32) != lat_s.view(torch.int32)).sum())} of {lat_s.numel()} latents differ in their bits"
    else:
        assert lat_c is None


def test_chain_ties_go_to_the_lowest_index():
    """Duplicated codebook rows (exact ties), as tests/test_hip_ndac.py builds them: the lower copy wins, in both kernels alike."""
    cfg = dict(NDAC75_LIKE, n_codebooks=6)
    sd = scaled_sd(cfg, 11, 0.75)
    for q in range(cfg["n_codebooks"]):
        cb = sd[f"quantizer.quantizers.{q}.codebook.weight"]
        cb[900:932] = cb[100:132]; cb[1000] = cb[3]
    from flowdec_amd.ndac import DAC
    m = DAC(**cfg); m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}); m = m.cuda()
    z = latent(m, 2, 509, 5)
    zq_s, codes_s, lat_s = run_steps(m, z, 6)
    zq_c, codes_c, lat_c = run_chain(m, z, 6)
    assert torch.equal(codes_c, codes_s) and same_bits(zq_c, zq_s) and same_bits(lat_c, lat_s)
    c = codes_c.cpu().numpy()
    assert not np.isin(c, np.r_[900:932, 1000]).any() and np.isin(c, np.r_[100:132, 3]).any()     # ties went to the lower copy
    zq_p, codes_p, lat_p = m.quantizer.encode_chain(z, 6)                                         # the Python surface is the same call
    assert torch.equal(codes_p, codes_c.long()) and same_bits(zq_p, zq_c) and same_bits(lat_p, lat_c)


@pytest.mark.parametrize("name", list(CFGS))
def test_chain_under_a_frame_table(name):
    m = model(name)
    T, frames = 23, (23, 9, 1)
    z = latent(m, 3, T, 7)
    alone = [run_chain(m, z[b:b + 1, :, :f].contiguous(), None) for b, f in enumerate(frames)]
    for b, f in enumerate(frames):                 # a one-clip dense call is the step launches' bits (the test above), here once more on the clip
        s = run_steps(m, z[b:b + 1, :, :f].contiguous(), None)
        assert all(same_bits(x, y) for x, y in zip(alone[b], s))
    zr = z.clone()
    for b, f in enumerate(frames):
        zr[b, :, f:] = float("nan")                # what lies behind a clip is never read as data
    zq, codes, lat = run_chain(m, zr, None, frames)
    for b, f in enumerate(frames):
        zq1, codes1, lat1 = alone[b]
        assert same_bits(zq[b:b + 1, :, :f], zq1) and torch.equal(codes[b:b + 1, :, :f], codes1) and same_bits(lat[b:b + 1, :, :f], lat1), f"row {b} ({f} frames)"
        for name_, t in (("z_q", zq), ("codes", codes), ("latents", lat)):
            assert torch.count_nonzero(t[b, :, f:]) == 0, f"{name_} of row {b} is not 0 behind frame {f}"
    assert torch.isfinite(zq).all() and torch.isfinite(lat).all() and int(codes.min()) >= 0
    # a device table and a host list agree (flowdec_amd.ndac ResidualVectorQuantize.encode_chain takes either)
    by_list = m.quantizer.encode_chain(zr, None, frames=list(frames))
    by_dev = m.quantizer.encode_chain(zr, None, frames=torch.tensor(frames, dtype=torch.int32, device="cuda"))
    assert torch.equal(by_list[1], codes.long()) and same_bits(by_list[0], zq) and same_bits(by_list[2], lat)
    assert all(same_bits(x, y) for x, y in zip(by_list, by_dev))
    full = run_chain(m, z, None, (T, T, T))        # every clip full: the dense call
    assert all(same_bits(x, y) for x, y in zip(full, run_chain(m, z, None)))


@pytest.mark.parametrize("bad", [(23, 0, 5), (23, 24, 5), (-1, 3, 5)])
def test_chain_refuses_bad_frame_counts_with_outputs_untouched(bad):
    from flowdec_amd import _lib as L
    m = model("ndac75")
    lib, T = L.load(), 23
    z = latent(m, 3, T, 7)
    zq = torch.full_like(z, 7.0)
    codes = torch.full((3, m.n_codebooks, T), -7, dtype=torch.int32, device="cuda")
    lat = torch.full((3, m.n_codebooks * m.codebook_dim, T), 7.0, device="cuda")
    fr = torch.tensor(bad, dtype=torch.int32, device="cuda")
    rc = lib.fd_rvq_encode_chain(m.handle(), L.ptr(z), L.ptr(fr), 3, T, 0, L.ptr(zq), L.ptr(codes), L.ptr(lat), L.stream())
    torch.cuda.synchronize()
    assert rc != 0 and b"frames[" in lib.fd_last_error()
    assert bool((zq == 7.0).all()) and bool((codes == -7).all()) and bool((lat == 7.0).all())
    with pytest.raises(RuntimeError, match="outside"):
        m.quantizer.encode_chain(z, None, frames=bad)
