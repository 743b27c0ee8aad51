#!/usr/bin/env python
"""Golden vectors for the time conditioning at model widths: the REFERENCE's GaussianFourierProjection(nf, scale=16), the two Linear
layers of the time embedding (ncsnpp.py:105-122, 263-274) and one ResnetBlockBigGANpp Dense_0 with the block's Conv_0.bias
(layerspp.py:236-239, 272-273), run on CPU in float32 at nf = 64 and nf = 128, eight times each.  Same import recipe as make_golden.py.

The inputs are NOT stored: tests/temb_ref.golden_inputs(nf) regenerates them from seeded NumPy, and the fixture holds their checksum.
Stored per nf: the checksum, temb [8][4 nf] and bias [8][33] = Conv_0.bias + Dense_0(silu(temb)) as the reference computes them from
its OWN temb.

    python tests/golden/make_golden_temb.py      # writes tests/golden/g34_temb.npz
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as MG  # noqa: E402  (stubs)
import temb_ref as R  # noqa: E402


def main():
    torch.set_grad_enabled(False)
    MG._install_stubs()
    from flowdec.backbones.ncsnpp_utils import layerspp

    out = {}
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    for nf in R.GOLDEN_NFS:
        g = R.golden_inputs(nf)
        gfp = layerspp.GaussianFourierProjection(embedding_size=nf, scale=16)
        gfp.W.data = T(g["W"])
        lin1, lin2 = torch.nn.Linear(2 * nf, 4 * nf), torch.nn.Linear(4 * nf, 4 * nf)
        dense = torch.nn.Linear(4 * nf, R.GOLDEN_COUT)
        for m, w, b in ((lin1, "w1", "b1"), (lin2, "w2", "b2"), (dense, "dw", "db")):
            m.weight.data, m.bias.data = T(g[w]), T(g[b])
        act = torch.nn.SiLU()
        temb = lin2(act(lin1(gfp(T(g["t"])))))
        bias = dense(act(temb)) + T(g["cb"])[None, :]
        out[f"nf{nf}_checksum"] = np.int64(R.checksum(g))
        out[f"nf{nf}_temb"] = temb.numpy()
        out[f"nf{nf}_bias"] = bias.numpy()
    np.savez_compressed(os.path.join(HERE, "g34_temb.npz"), **out)
    print({k: getattr(v, "shape", v) for k, v in out.items()})


if __name__ == "__main__":
    main()
