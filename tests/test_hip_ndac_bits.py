"""The codec's outputs, bit for bit, against recorded hashes: a change to how ndac.hip walks its layers, sizes its workspace or picks a
kernel must leave every byte of encode / decode / their ragged forms / from_codes where it was.

tests/golden/ndac_bits.json holds SHA-256 digests written by this file's `__main__` (`python tests/test_hip_ndac_bits.py [OUT.json]`) on an
MI355X at commit e828d71, the last one whose ndac.hip spelled the encoder and decoder stacks out by hand.  Every kernel accumulates in a
fixed order, so the digests do not depend on the run.  The configurations are the smallest that cross every branch of the walks: the first
convolution, three dilations, strided and transposed convolutions with even and odd strides, kept and dropped raw outputs, the tanh layer,
the zero-tail kernel, both quantiser paths and both precisions."""
import hashlib
import json
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)                    # (run as a script: `oracle` and the package are imported from the tree)
from test_ndac_cpu import SMALL, scaled_sd      # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ndac_bits.json")
CONFIGS = {
    "small_direct": (SMALL, "mfma_decoder"),                                  # no layer wide enough for the matrix cores; odd stride 5
    "decoder256_mfma": (dict(SMALL, decoder_dim=256), "mfma_decoder"),        # the decoder on the matrix cores, transposed layers included
    "encoder32_mfma": (dict(SMALL, encoder_dim=32), "mfma"),                  # the encoder on the matrix cores
}
FRAMES = [7, 3]


def digest(t):
    return hashlib.sha256(np.ascontiguousarray(t.detach().cpu().numpy()).tobytes()).hexdigest()


def run_config(cfg, precision):
    from flowdec_amd.ndac import DAC
    m = DAC(**cfg, precision=precision)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in scaled_sd(cfg, 3, 0.7).items()})
    m = m.to("cuda")
    rng = np.random.default_rng(11)
    x = torch.from_numpy((0.3 * rng.standard_normal((2, 1, 7 * m.hop_length))).astype(np.float32)).to("cuda")
    out = {}
    z, codes, lat, _, _ = m.encode(x)
    out.update(encode_z=digest(z), encode_codes=digest(codes), encode_latents=digest(lat))
    zr, cr, lr = m.encode_ragged(x, FRAMES)
    out.update(encode_ragged_z=digest(zr), encode_ragged_codes=digest(cr), encode_ragged_latents=digest(lr))
    out["decode"] = digest(m.decode(z))
    out["decode_ragged"] = digest(m.decode_ragged(z, FRAMES))
    out["from_codes"] = digest(m.quantizer.from_codes(codes)[0])
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_bits_equal_the_recorded_ones(name):
    with open(GOLDEN) as f:
        golden = json.load(f)
    assert "e828d71" in golden["source"]
    got = run_config(*CONFIGS[name])
    want = golden["digests"][name]
    assert set(got) == set(want) and len(got) == 9
    differ = sorted(k for k in got if got[k] != want[k])
    print(f"ndac_bits[{name}]: {len(got) - len(differ)} of {len(got)} outputs keep their recorded bits")
    assert not differ, f"{name}: {differ} changed their bits"


if __name__ == "__main__":
    import subprocess
    import __graft_entry__ as g
    g.build()
    rev = subprocess.run(["git", "rev-parse", "--short", "HEAD"], cwd=ROOT, capture_output=True, text=True).stdout.strip() or "unknown"
    res = {"source": (sys.argv[2] if len(sys.argv) > 2 else rev), "digests": {name: run_config(*CONFIGS[name]) for name in sorted(CONFIGS)}}
    with open(sys.argv[1] if len(sys.argv) > 1 else GOLDEN, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
    print(json.dumps(res, sort_keys=True))
