"""Bit-identity of the F(4,3) bf16 kernel (conv_wino4.hip) on the halo shapes tests/test_wino4_onepass.py lacks.

The producer pass of the kernel builds the 18 halo rows x 18 halo columns of a chunk; any change of how the rows and columns are
spread over the lanes must keep every V word the same function of the same bytes in the same operation order, so the outputs AND the
GroupNorm partial sums of fd_conv2d(FD_WINOGRAD4) keep their bits.  tests/golden/g28_wino4_rows.json holds, per case, the SHA-256 of
the output bytes and of the statistics bytes as the library of the commit BEFORE the balanced pass (a 4-tile item mapping with a second
pass on one wave for halo rows 16 and 17) produced them on an MI355X (recorded once with `python tests/test_wino4_rows.py --record FILE`
under that library), plus a strided sample of both so that a mismatch can be located.  The
inputs are integers from numpy's frozen RandomState scaled by powers of two: the same bits on every machine.

Shapes (what g27 does not reach):
  16x32  at B = 1   two tile columns: the left and the right column mask each next to a neighbouring tile
  48x16  at B = 1   three tile rows: halo rows 16 and 17 valid (top and middle tile) and masked at the bottom of the image
  Cin 160 at B = 2  five chunk pairs (32x32: interior corners of four tiles)
each with ACT on and off x {plain, residual (SKIP), folded shortcut (SC, 64 channels)} x both tile orders (FD_TILE_REVERSED)."""
import hashlib
import json
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN_FILE = os.path.join(HERE, "golden", "g28_wino4_rows.json")
COUT = 256
SAMPLE_STRIDE = 4099

# name -> (B, H, W, Cin)
SHAPES = {
    "16x32": (1, 16, 32, 64),
    "48x16": (1, 48, 16, 64),
    "cin160": (2, 32, 32, 160),
}
KINDS = ("plain", "skip", "sc")
# (act, reversed)
MODES = [(a, r) for a in (False, True) for r in (False, True)]


def _ints(rs, shape, lo, hi, scale):
    return (rs.randint(lo, hi, size=shape).astype(np.float32) * np.float32(scale))


def make_case(shape, kind, act):
    """Host tensors of one case (all values exact in bf16 / f32: integers times powers of two)."""
    B, H, W, Cin = SHAPES[shape]
    rs = np.random.RandomState(28000 + 100 * sorted(SHAPES).index(shape) + 10 * KINDS.index(kind) + int(act))
    c = {"x": _ints(rs, (B, H, W, Cin), -128, 128, 2.0 ** -5), "w": _ints(rs, (COUT, Cin, 3, 3), -64, 64, 2.0 ** -10),
         "bias": _ints(rs, (COUT,), -64, 64, 2.0 ** -6)}
    if act:
        c["affine"] = np.stack([1.0 + _ints(rs, (B, Cin), -64, 64, 2.0 ** -8), _ints(rs, (B, Cin), -64, 64, 2.0 ** -7)], -1).astype(np.float32)
    if kind == "skip":
        c["skip"] = _ints(rs, (B, H, W, COUT), -128, 128, 2.0 ** -5)
    if kind == "sc":
        c["sc"] = _ints(rs, (B, H, W, 64), -128, 128, 2.0 ** -5)
        c["w_sc"] = _ints(rs, (COUT, 64, 1, 1), -64, 64, 2.0 ** -8)
    return c


def run_case(ops, shape, kind, act, rev):
    """(output bytes, statistics bytes) of fd_conv2d(FD_WINOGRAD4) on the case."""
    c = make_case(shape, kind, act)
    dev = lambda v, dt=torch.float32: torch.from_numpy(np.ascontiguousarray(v)).to("cuda").to(dt).contiguous()
    bf = torch.bfloat16
    w_sc = dev(c["w_sc"]) if kind == "sc" else None
    pw = ops.pack_conv_weight(dev(c["w"]), dtype=bf, w_sc=w_sc, S0=64 if kind == "sc" else None, winograd=4)
    out, st = ops.conv2d(dev(c["x"], bf), pw, COUT, 3, affine=dev(c["affine"]) if act else None, bias=dev(c["bias"]),
                         skip=dev(c["skip"], bf) if kind == "skip" else None, scale=0.7071, sc0=dev(c["sc"], bf) if kind == "sc" else None,
                         want_stats=True, winograd=4, reversed_tiles=rev)
    torch.cuda.synchronize()
    return out.view(torch.int16).cpu().numpy(), st.view(torch.int32).cpu().numpy()


def digest(out, st):
    return {"out_sha256": hashlib.sha256(out.tobytes()).hexdigest(), "stats_sha256": hashlib.sha256(st.tobytes()).hexdigest(),
            "out_sample": [int(v) for v in out.ravel()[::SAMPLE_STRIDE]], "stats_sample": [int(v) for v in st.ravel()[::SAMPLE_STRIDE]]}


def case_id(shape, kind, act, rev):
    return f"{shape}/{kind}/act{int(act)}/rev{int(rev)}"


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
def test_bits_of_recorded_library(ops, recorded, shape, kind):
    bad = []
    for act, rev in MODES:
        cid = case_id(shape, kind, act, rev)
        got, want = digest(*run_case(ops, shape, kind, act, rev)), recorded[cid]
        if got != want:
            ns = sum(a != b for a, b in zip(got["out_sample"], want["out_sample"]))
            nt = sum(a != b for a, b in zip(got["stats_sample"], want["stats_sample"]))
            bad.append(f"{cid}: output {'differs' if got['out_sha256'] != want['out_sha256'] else 'same'} ({ns} of {len(want['out_sample'])} "
                       f"sampled values), statistics {'differ' if got['stats_sha256'] != want['stats_sha256'] else 'same'} ({nt} sampled)")
    assert not bad, "not the bits of the recorded library:\n" + "\n".join(bad)


def test_every_case_is_recorded(recorded):
    """36 cases: three shapes x three kinds x ACT on / off x both tile orders, each with both digests."""
    want = {case_id(s, k, a, r) for s in SHAPES for k in KINDS for a, r in MODES}
    assert set(recorded) == want and len(want) == 36
    assert all(len(v["out_sha256"]) == 64 and len(v["stats_sha256"]) == 64 for v in recorded.values())


def test_reversed_order_has_the_same_output_bits(recorded):
    """The tile order changes which workgroup computes a tile, not what it computes: both orders were recorded with the same digests."""
    for s in SHAPES:
        for k in KINDS:
            for a in (False, True):
                assert recorded[case_id(s, k, a, False)] == recorded[case_id(s, k, a, True)]


if __name__ == "__main__":   # python tests/test_wino4_rows.py --record FILE | --compare FILE   (FLOWDEC_HIP_LIB selects the library)
    sys.path.insert(0, os.path.dirname(HERE))
    from flowdec_amd import ops as _ops
    mode, path = sys.argv[1], sys.argv[2]
    cases = {}
    for shape in SHAPES:
        for kind in KINDS:
            for act, rev in MODES:
                cases[case_id(shape, kind, act, rev)] = digest(*run_case(_ops, shape, kind, act, rev))
    if mode == "--record":
        with open(path, "w") as f:
            json.dump({"kernel": "conv_wino4_kernel, one-pass producer with the second pass of wave 1 for halo rows 16 and 17", "cases": cases}, f, indent=0)
        print("recorded", len(cases), "cases ->", path)
    else:
        with open(path) as f:
            want = json.load(f)["cases"]
        diff = [k for k in cases if cases[k] != want[k]]
        print("compared", len(cases), "cases:", "ALL IDENTICAL" if not diff else f"{len(diff)} DIFFER: {diff[:20]}")
        sys.exit(1 if diff else 0)
