"""Bit-identity of the F(4,3) bf16 kernel (conv_wino4.hip) with its one-pass producer against the library of the commit before it.

The one-pass producer (RAW halo -> registers -> V planes, no activated-halo staging buffer) computes every V word with the same
function and the same operation order as the two-stage producer it replaces: only the staging changed.  So the outputs AND the
GroupNorm partial sums of fd_conv2d(FD_WINOGRAD4) must keep their bits.  tests/golden/g27_wino4_onepass.json holds, per case, the
SHA-256 of the output bytes and of the statistics bytes as the PREVIOUS commit's library produced them on an MI355X (recorded once
with `python tests/test_wino4_onepass.py --record FILE` under that library), plus a strided sample of both so that a mismatch can
be located.  The inputs are integers from numpy's frozen RandomState scaled by powers of two: the same bits on every machine.

Shapes (the smallest that reach every path of the producer; B = 2 unless noted):
  16x16            one tile, all four borders masked
  32x48            interior and edge tiles, rows 16 / 17 of the halo in use
  16x16 at B = 3   band addressing across images
  Cin 32           one chunk pair
  Cin 96           an odd number of chunk pairs (see below)
  Cin 256 + 64     a two-segment concat (affine table offset across segments)
each with ACT on and off x {plain, residual (SKIP), folded shortcut (SC, 64 channels)} x both tile orders (FD_TILE_REVERSED), and
one input with values beyond RAW_MAX = 6000 (the saturation: the fmed3 of the raw path, and with ACT the min behind silu(a x + d) on
the positive side and silu(-8000) = -0 on the negative one).

Cin 48 (an odd CHUNK count, a half-used last pair) is not a shape fd_conv2d accepts for this kernel: FD_WINOGRAD4 with bf16 storage
requires channel counts that are multiples of 32 (fd_wino4_supported), before and after this change.  test_cin48_is_refused pins
that; Cin 96 covers the nearest reachable case."""
import hashlib
import json
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN_FILE = os.path.join(HERE, "golden", "g27_wino4_onepass.json")
COUT = 256
SAMPLE_STRIDE = 4099

# name -> (B, H, W, C0, C1)
SHAPES = {
    "16x16": (2, 16, 16, 64, 0),
    "32x48": (2, 32, 48, 64, 0),
    "16x16_b3": (3, 16, 16, 64, 0),
    "cin32": (2, 32, 48, 32, 0),
    "cin96": (2, 32, 48, 96, 0),
    "cat256+64": (2, 32, 48, 256, 64),
}
KINDS = ("plain", "skip", "sc")
# (act, reversed, saturating input)
MODES = [(a, r, False) for a in (False, True) for r in (False, True)] + [(False, False, True), (True, False, True)]


def _ints(rs, shape, lo, hi, scale):
    return (rs.randint(lo, hi, size=shape).astype(np.float32) * np.float32(scale))


def make_case(shape, kind, act, sat):
    """Host tensors of one case (all values exact in bf16 / f32: integers times powers of two)."""
    B, H, W, C0, C1 = SHAPES[shape]
    Cin = C0 + C1
    rs = np.random.RandomState(1000 * sorted(SHAPES).index(shape) + 10 * KINDS.index(kind) + 2 * int(act) + int(sat))
    x = _ints(rs, (B, H, W, Cin), -128, 128, 2.0 ** -5)
    a = 1.0 + _ints(rs, (B, Cin), -64, 64, 2.0 ** -8)
    d = _ints(rs, (B, Cin), -64, 64, 2.0 ** -7)
    if sat:   # |x| up to 8192 > RAW_MAX on every fourth channel
        big = np.arange(Cin) % 4 == 1
        x[..., big] = _ints(rs, (B, H, W, int(big.sum())), -128, 128, 64.0)
    c = {"x": x, "w": _ints(rs, (COUT, Cin, 3, 3), -64, 64, 2.0 ** -10), "bias": _ints(rs, (COUT,), -64, 64, 2.0 ** -6)}
    if act:
        c["affine"] = np.stack([a, d], -1).astype(np.float32)
    if kind == "skip":
        c["skip"] = _ints(rs, (B, H, W, COUT), -128, 128, 2.0 ** -5)
    if kind == "sc":
        c["sc"] = _ints(rs, (B, H, W, 64), -128, 128, 2.0 ** -5)
        c["w_sc"] = _ints(rs, (COUT, 64, 1, 1), -64, 64, 2.0 ** -8)
    return c


def run_case(ops, shape, kind, act, rev, sat):
    """(output bytes, statistics bytes) of fd_conv2d(FD_WINOGRAD4) on the case."""
    B, H, W, C0, C1 = SHAPES[shape]
    c = make_case(shape, kind, act, sat)
    dev = lambda v, dt=torch.float32: torch.from_numpy(np.ascontiguousarray(v)).to("cuda").to(dt).contiguous()
    bf = torch.bfloat16
    x = dev(c["x"], bf)
    x0 = x[..., :C0].contiguous()
    x1 = x[..., C0:].contiguous() if C1 else None
    w_sc = dev(c["w_sc"]) if kind == "sc" else None
    pw = ops.pack_conv_weight(dev(c["w"]), C0=C0, dtype=bf, w_sc=w_sc, S0=64 if kind == "sc" else None, winograd=4)
    out, st = ops.conv2d(x0, pw, COUT, 3, x1=x1, affine=dev(c["affine"]) if act else None, bias=dev(c["bias"]),
                         skip=dev(c["skip"], bf) if kind == "skip" else None, scale=0.7071, sc0=dev(c["sc"], bf) if kind == "sc" else None,
                         want_stats=True, winograd=4, reversed_tiles=rev)
    torch.cuda.synchronize()
    return out.view(torch.int16).cpu().numpy(), st.view(torch.int32).cpu().numpy()


def digest(out, st):
    return {"out_sha256": hashlib.sha256(out.tobytes()).hexdigest(), "stats_sha256": hashlib.sha256(st.tobytes()).hexdigest(),
            "out_sample": [int(v) for v in out.ravel()[::SAMPLE_STRIDE]], "stats_sample": [int(v) for v in st.ravel()[::SAMPLE_STRIDE]]}


def case_id(shape, kind, act, rev, sat):
    return f"{shape}/{kind}/act{int(act)}/rev{int(rev)}/sat{int(sat)}"


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.fail("needs a GPU")
    from flowdec_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def recorded():
    with open(GOLDEN_FILE) as f:
        return json.load(f)["cases"]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_bits_of_previous_library(ops, recorded, shape, kind):
    bad = []
    for act, rev, sat in MODES:
        cid = case_id(shape, kind, act, rev, sat)
        got, want = digest(*run_case(ops, shape, kind, act, rev, sat)), recorded[cid]
        if got != want:
            ns = sum(a != b for a, b in zip(got["out_sample"], want["out_sample"]))
            nt = sum(a != b for a, b in zip(got["stats_sample"], want["stats_sample"]))
            bad.append(f"{cid}: output {'differs' if got['out_sha256'] != want['out_sha256'] else 'same'} ({ns} of {len(want['out_sample'])} "
                       f"sampled values), statistics {'differ' if got['stats_sha256'] != want['stats_sha256'] else 'same'} ({nt} sampled)")
    assert not bad, "not the bits of the previous library:\n" + "\n".join(bad)


def test_saturating_cases_saturate():
    """The `sat` inputs do hold values beyond RAW_MAX on both sides, before and behind the affine (host-side premise of the cases)."""
    for act in (False, True):
        c = make_case("16x16", "plain", act, True)
        u = c["x"] * c["affine"][:, None, None, :, 0] + c["affine"][:, None, None, :, 1] if act else c["x"]
        assert u.max() > 6000.0 and u.min() < -6000.0 and np.abs(u).max() < 60000.0


def test_cin48_is_refused(ops):
    """FD_WINOGRAD4 in bf16 takes channel counts that are multiples of 32 only: an odd chunk count does not reach the kernel."""
    w = torch.zeros(COUT, 48, 3, 3, device="cuda")
    with pytest.raises(RuntimeError):
        pw = ops.pack_conv_weight(w, dtype=torch.bfloat16, winograd=4)
        ops.conv2d(torch.zeros(2, 16, 16, 48, device="cuda", dtype=torch.bfloat16), pw, COUT, 3, winograd=4)


if __name__ == "__main__":   # python tests/test_wino4_onepass.py --record FILE | --compare FILE   (FLOWDEC_HIP_LIB selects the library)
    sys.path.insert(0, os.path.dirname(HERE))
    from flowdec_amd import ops as _ops
    mode, path = sys.argv[1], sys.argv[2]
    cases = {}
    for shape in SHAPES:
        for kind in KINDS:
            for act, rev, sat in MODES:
                cases[case_id(shape, kind, act, rev, sat)] = digest(*run_case(_ops, shape, kind, act, rev, sat))
    if mode == "--record":
        with open(path, "w") as f:
            json.dump({"kernel": "conv_wino4_kernel, two-stage producer (the commit before the one-pass producer)", "cases": cases}, f, indent=0)
        print("recorded", len(cases), "cases ->", path)
    else:
        with open(path) as f:
            want = json.load(f)["cases"]
        diff = [k for k in cases if cases[k] != want[k]]
        print("compared", len(cases), "cases:", "ALL IDENTICAL" if not diff else f"{len(diff)} DIFFER: {diff[:20]}")
        sys.exit(1 if diff else 0)
