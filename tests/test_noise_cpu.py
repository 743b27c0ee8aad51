"""Seeded sampler noise, host side: the oracle's Philox against the Random123 known answers, the clip-seed mix, the declared ABI
and the argument checks of the Python surface (no GPU needed)."""
import os
import re

import numpy as np
import pytest
import torch

import noise_oracle as NO
from conftest import ROOT

KAT = [   # Random123 kat_vectors, philox4x32-10: counter, key -> output
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
]


@pytest.mark.parametrize("ctr,key,want", KAT)
def test_oracle_philox_known_answers(ctr, key, want):
    assert tuple(int(x) for x in NO.philox4x32_10(*ctr, *key)) == want


def test_oracle_plane_layout():
    """Frames 2k and 2k + 1 share one Philox call; a plane does not depend on its width (also an odd one)."""
    ra, rb = NO.noise_bits(1000, 3, 4, 10)
    r = NO.philox4x32_10(2, 1, 3, 0, 1000, 0)
    assert (int(ra[1, 4]), int(rb[1, 4]), int(ra[1, 5]), int(rb[1, 5])) == tuple(int(x) for x in r)
    a, b = NO.noise_bits(1000, 3, 4, 7)
    assert np.array_equal(a, ra[:, :7]) and np.array_equal(b, rb[:, :7])
    hi = NO.noise_bits((5 << 32) | 1000, 3, 4, 10)[0]
    assert not np.array_equal(hi, ra)                      # the high key word matters
    z = NO.noise_plane(1000, 0, 8, 64)
    assert np.abs(z).max() <= np.sqrt(24 * np.log(2)) + 1e-12


def test_clip_seed_has_no_collisions():
    from flowdec_amd.noise import clip_seed
    grid = {(s, i): clip_seed(s, i) for s in range(64) for i in range(64)}
    assert len(set(grid.values())) == 64 * 64
    assert all(0 <= v < 1 << 64 for v in grid.values())
    for s in range(63):
        for i in range(63):
            assert grid[(s, i + 1)] != grid[(s + 1, i)]
    assert clip_seed(-1, 0) == clip_seed((1 << 64) - 1, 0)   # a seed is taken modulo 2^64


def test_seeds_to_tensor():
    from flowdec_amd.noise import clip_seed, seeds_to_tensor
    t = seeds_to_tensor(5, 3, "cpu")
    assert t.dtype == torch.int64 and [int(v) & ((1 << 64) - 1) for v in t] == [clip_seed(5, b) for b in range(3)]
    assert [int(v) for v in seeds_to_tensor([1, (1 << 64) - 1], 2, "cpu")] == [1, -1]
    assert torch.equal(seeds_to_tensor(torch.tensor([7, 8]), 2, "cpu"), torch.tensor([7, 8]))
    with pytest.raises(RuntimeError):
        seeds_to_tensor([1, 2, 3], 2, "cpu")
    with pytest.raises(RuntimeError):
        seeds_to_tensor(torch.tensor([1.0, 2.0]), 2, "cpu")


def test_seeded_symbols_declared_with_signatures():
    from flowdec_amd import _lib
    src = open(os.path.join(ROOT, "include", "flowdec_hip.h")).read()
    decl = set(re.findall(r"\b(fd_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", src, flags=re.S)))
    for name in ("fd_noise_fill", "fd_ode_solve_seeded", "fd_enhance_seeded", "fd_score_enhance_seeded"):
        assert name in decl, f"{name} is not declared in include/flowdec_hip.h"
        assert name in _lib.SIGNATURES, f"{name} has no ctypes signature"
        assert hasattr(_lib.load(), name), f"{name} is not exported"
    assert "FD_NOISE_GAUSSIAN 0" in src and "FD_NOISE_BITS 1" in src


def test_noise_sources_are_exclusive():
    import flowdec_amd
    from flowdec_amd.dist import sharded_enhance
    y = torch.zeros(1, 1, 4800)
    nz = torch.zeros(1, 1, 768, 64, dtype=torch.complex64)
    m = flowdec_amd.from_preset("flowdec_75m", nf=8)
    with pytest.raises(ValueError, match="only one"):
        m.enhance(y, seed=1, noise=nz)
    with pytest.raises(ValueError, match="only one"):
        m.enhance(y, seed=1, generator=torch.Generator())
    with pytest.raises(ValueError, match="only one"):
        m.enhance_batch([y], seeds=[1], noise=[nz])
    s = flowdec_amd.from_preset("baseline_scoredec_75s", nf=8)
    with pytest.raises(ValueError, match="only one"):
        s.enhance(y, seed=1, noise=nz)
    with pytest.raises(ValueError, match="native"):
        sharded_enhance(m, y, rng="native", seed=1, noise=nz)
    with pytest.raises(ValueError, match="rng"):
        sharded_enhance(m, y, rng="bogus")


def test_cli_parser_accepts_rng():
    from flowdec_amd import enhance_cli
    base = ["--ckpt", "a", "--files", "b", "--outdir", "c", "--N", "1"]
    p = enhance_cli.build_parser()
    assert p.parse_args(base).rng == "torch"
    assert p.parse_args(base + ["--rng", "native", "--seed", "3"]).rng == "native"
    with pytest.raises(SystemExit):
        p.parse_args(base + ["--rng", "bogus"])
