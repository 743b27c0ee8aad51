#!/usr/bin/env python
"""Golden vectors for the validation loss: the REFERENCE's FlowModel._loss, ScoreModel._loss and RegressionModel._loss
(flowdec/model.py:421-468, :590-611, :552-559) run on CPU.  Same import recipe and the same seeded nf = 8 weights as make_golden.py /
make_golden_score.py.  The random draws are replaced: torch.rand returns the recorded `t`-uniforms stored here, torch.randn_like returns
the seeded NumPy stream `oracle.seeded_noises(NOISE_SEED, shape)`, which the tests regenerate (draw 0 = Ys' noise, draw 1 = Xs' noise,
in the order `_loss` calls it).

torchcfm is not installed where this script runs.  `StandInCFM` below is a STAND-IN for torchcfm.ConditionalFlowMatcher with sigma = 0:
xt = t x1 + (1 - t) x0, ut = x1 - x0 (its sample_location_and_conditional_flow with the noise term sigma * eps dropped) -- NOT the real
package.  The score and regression cases need none.

Stored per case: t, the reference's per-clip values before its reduction and its final loss (float32, as it computes them), and, from
the reference's own network output V_ref and target in float64, the per-clip sums  sum |err|^2,  ||V_ref||^2 (the tolerance of the GPU
test is derived from these two).  For ONE flow case (curve sigma_y, sigma_x = 0.1) the reference's own Ymu, Xmu, Xt and Ut of clip 1 (the
clip scaled by 2.5) at every 4th frequency row and all 64 frames: the state arithmetic is elementwise, so the sub-grid checks it against
the reference's own spectrograms, and the full planes would put the file over the size limit for a committed file.

    python tests/golden/make_golden_loss.py      # writes tests/golden/g33_valid_loss.npz
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG  # noqa: E402  (stubs + helpers)
from oracle import flowdec_oracle as O  # noqa: E402

NOISE_SEED = 3333
FLOW_CASES = {  # name -> (sigma_y: 'scalar' | 'curve', sigma_x)
    "flow_scalar_sx0": ("scalar", 0.0),
    "flow_scalar_sx01": ("scalar", 0.1),
    "flow_curve_sx0": ("curve", 0.0),
    "flow_curve_sx01": ("curve", 0.1),
}
STATE_CASE = "flow_curve_sx01"
STATE_FSTRIDE = 4   # the stored state arrays hold every 4th frequency row


class StandInCFM:
    """STAND-IN for torchcfm.ConditionalFlowMatcher(sigma=0): not the real package."""
    sigma = 0.0

    def sample_location_and_conditional_flow(self, x0, x1, t=None):
        tb = t.reshape(-1, *([1] * (x0.dim() - 1)))
        xt = tb * x1 + (1 - tb) * x0
        ut = x1 - x0
        return t, xt, ut


def main():
    torch.manual_seed(0)
    torch.set_grad_enabled(False)
    MG._install_stubs()
    from flowdec.backbones.ncsnpp import NCSNpp
    from flowdec.data import sigma_models
    from flowdec.data.feature_extractors import AmplitudeCompressedComplexSTFT
    from flowdec.model import FlowModel, RegressionModel, ScoreModel
    from flowdec.sdes import OUVESDE
    bb_kw = dict(nonlinearity="swish", ch_mult=(4, 4, 4, 2), num_res_blocks=1, attn_resolutions=[], resamp_with_conv=True,
                 conditional=True, fir=True, fir_kernel=[1, 3, 3, 1], skip_rescale=True, resblock_type="biggan",
                 progressive="output_skip", progressive_input="input_skip", progressive_combine="sum", init_scale=0.0,
                 fourier_scale=16, image_size=768, embedding_type="fourier", dropout=0.0, num_channels=4,
                 output_layer_kwargs=dict(kernel_size=1, bias=False, padding="same", padding_mode="zeros"),
                 bottleneck_attn=False)   # config/model/backbone/ncsnpp_final_no_attn.yaml
    fe = AmplitudeCompressedComplexSTFT(window_fn="hann", n_fft=1534, n_hops=4, sampling_rate=48000, alpha=0.3, beta=0.33)
    sd8 = O.random_state_dict(seed=8, nf=8)
    backbone = NCSNpp(nf=8, **bb_kw).eval()
    backbone.load_state_dict(MG.to_t(MG.strip(sd8, "backbone.")))
    common = dict(backbone=backbone, feature_extractor=fe, sampling_rate=48000, lr=1e-4, full_config={})

    rng = np.random.default_rng(33)
    L, B = 12000, 2
    x = (0.1 * rng.standard_normal((B, 1, L))).astype(np.float32)
    y = (x + 0.03 * rng.standard_normal((B, 1, L))).astype(np.float32)   # a "coded" signal close to the clean one
    x[1] *= 2.5; y[1] *= 2.5
    Tp = O.padded_frames(O.num_frames(L))
    u = rng.random(B).astype(np.float32)          # what torch.rand(B) returns
    curve = sigma_models.from_file(os.path.join(MG.REF, "data", "flowdec_autoparams_75m.npy"), factor=1, kernel_bandwidth=3)
    out = dict(x=x, y=y, u=u, noise_seed=np.int64(NOISE_SEED), weight_seed=np.int64(8), sde=np.array([1.5, 0.05, 0.5]), t_eps=np.float64(3e-2),
               sigma_y_scalar=np.float64(0.66), sigma_y_curve=curve.numpy(), state_case=np.array(STATE_CASE))
    batch = (torch.from_numpy(x), torch.from_numpy(y), ["clip0", "clip1"])
    real_rand, real_randn_like = torch.rand, torch.randn_like

    def run(name, model, n_draws):
        """model._loss on the batch with the draws replaced; records what the forward pass saw and returned."""
        stream = O.seeded_noises(NOISE_SEED, (B, 1, 768, Tp))
        drawn, seen = [0], {}

        def fake_randn_like(t, *a, **k):
            assert tuple(t.shape) == (B, 1, 768, Tp) and t.dtype == torch.complex64
            drawn[0] += 1
            return torch.from_numpy(next(stream))

        def fake_rand(*shape, **k):
            assert tuple(shape) == (B,)
            return torch.from_numpy(u.copy())
        orig_forward = type(model).forward

        def spy(self, xt, yy, t):
            seen["xt"], seen["t"] = xt.clone(), t.clone()
            seen["v"] = orig_forward(self, xt, yy, t)
            return seen["v"]
        torch.rand, torch.randn_like = fake_rand, fake_randn_like
        type(model).forward = spy
        try:
            loss = model._loss(batch, 0, "valid")
        finally:
            torch.rand, torch.randn_like = real_rand, real_randn_like
            type(model).forward = orig_forward
        assert drawn[0] == n_draws, (name, drawn[0])
        out[name + "_loss"] = loss.numpy()
        out[name + "_t"] = seen["t"].numpy().astype(np.float32)
        return seen

    def sums64(err):
        e = err.numpy().astype(np.complex128).reshape(B, -1)
        return (e.real ** 2 + e.imag ** 2).sum(axis=1)

    # ---- flow ----------------------------------------------------------------------------------------------------------------------
    for name, (sy, sx) in FLOW_CASES.items():
        fm = FlowModel(flow_matcher=StandInCFM(), sigma_x=sx, sigma_y=(0.66 if sy == "scalar" else curve), **common).eval()
        fm.error_weighting = None     # _loss reads it (model.py:439); EnhancementModel.__init__ never sets it
        seen = run(name, fm, 2)       # sigma_x is a Parameter there, so _get_noise draws for Xs even at sigma_x = 0 (and multiplies by 0)
        # Ut is not an argument of forward(): rebuild the target from the same expressions (model.py:431-433)
        Ymu, Xmu, _ = fm._preprocess(batch[1], x=batch[0])
        stream = O.seeded_noises(NOISE_SEED, (B, 1, 768, Tp))
        z0, z1 = torch.from_numpy(next(stream)), torch.from_numpy(next(stream))
        Ys = Ymu + (fm.sigma_y * z0).type(Ymu.dtype)
        Xs = Xmu + (fm.sigma_x * z1).type(Xmu.dtype)
        _, Xt, Ut = fm.flow_matcher.sample_location_and_conditional_flow(Ys, Xs, t=seen["t"])
        assert torch.equal(torch.view_as_real(Xt), torch.view_as_real(seen["xt"]))
        err = seen["v"] - Ut
        out[name + "_per_clip"] = (err.abs() ** 2).flatten(start_dim=1).mean(dim=1).numpy()
        out[name + "_sums"] = sums64(err)
        out[name + "_vnorm2"] = sums64(seen["v"])
        if name == STATE_CASE:
            sub = lambda a: np.ascontiguousarray(a[1:2, :, ::STATE_FSTRIDE].numpy())
            out["state_Y"], out["state_X"], out["state_Xt"], out["state_Ut"] = sub(Ymu), sub(Xmu), sub(Xt), sub(Ut)
            out["state_fstride"] = np.int64(STATE_FSTRIDE)
        print(name, "t", seen["t"].numpy(), "loss", float(out[name + "_loss"]), "per clip", out[name + "_per_clip"])

    # ---- score ---------------------------------------------------------------------------------------------------------------------
    sm = ScoreModel(sde=OUVESDE(theta=1.5, sigma_min=0.05, sigma_max=0.5, N=30), t_eps=3e-2, **common).eval()
    seen = run("score", sm, 1)
    z0 = torch.from_numpy(next(O.seeded_noises(NOISE_SEED, (B, 1, 768, Tp))))
    std = sm.sde._std(seen["t"])[:, None, None, None]
    err = std * (seen["v"] - (-z0 / std))          # seen["v"] is the score estimate -backbone / std (model.py:626-628)
    out["score_per_clip"] = torch.square(err.abs()).reshape(B, -1).sum(dim=-1).numpy()
    out["score_sums"] = sums64(err)
    out["score_vnorm2"] = sums64(-seen["v"] * std)  # the backbone's own output
    out["score_std"] = std.reshape(B).numpy()
    print("score t", seen["t"].numpy(), "loss", float(out["score_loss"]), "per clip", out["score_per_clip"])

    # ---- regression ----------------------------------------------------------------------------------------------------------------
    rm = RegressionModel(loss_type="l2", **common).eval()
    seen = run("regression", rm, 0)
    _, X, _ = rm._preprocess(batch[1], x=batch[0])
    err = seen["v"] - X
    out["regression_per_clip"] = (err.abs() ** 2).flatten(start_dim=1).mean(dim=1).numpy()
    out["regression_sums"] = sums64(err)
    out["regression_vnorm2"] = sums64(seen["v"])
    print("regression loss", float(out["regression_loss"]), "per clip", out["regression_per_clip"])

    path = os.path.join(HERE, "g33_valid_loss.npz")
    np.savez_compressed(path, **out)
    print("g33_valid_loss.npz", os.path.getsize(path) / 1024, "KiB")


if __name__ == "__main__":
    main()
