#!/usr/bin/env python
"""One-command pinning kit for the two THIRD-PARTY pieces of the FlowDec inference path that are absent from the offline build
container: `torchdyn==1.0.6` (the ODE driver behind FlowModel.enhance, reference requirements.txt:53,
flowdec/model.py:503-515) and `descript-audio-codec==1.0.0` (the NDAC codec of demo.ipynb cells 2-3, requirements.txt:4).

    pip install torchdyn==1.0.6 descript-audio-codec==1.0.0        # needs a network
    python scripts/pin_third_party.py                              # CPU only; writes tests/golden/g_pin_*.npz and a report

For every package that imports, the oracle's restatement (oracle/flowdec_oracle.py: odeint_fixed / odeint_adaptive / the NeuralODE
default tolerances; oracle/ndac_oracle.py: DACOracle) is compared with the REAL package on seeded inputs, golden vectors produced by the
real package are written next to the existing fixtures, and a JSON report says PINNED / MISMATCH per item.  Packages that do not import
are reported as "absent" and skipped (exit status 0): that is the state of the offline container, where this script cannot pin anything.
tests/test_pin_third_party.py runs the same checks under pytest (skipped when both packages are absent).

Rows this flips in DESIGN.md section 1 once it has run green somewhere: f4 (adaptive solvers, driver semantics of a6) and f2 (NDAC).
Row f4 also records a one-ulp difference in the stage times between the oracle's `dopri5_adapt_step` (float32 product under NumPy 2) and
the library's `StepCtl::end` (double product, rounded once): the adaptive comparison here says which of the two is torchdyn's."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden")


def have(mod):
    try:
        __import__(mod)
        return True
    except Exception:
        return False


# ------------------------------------------------------------------------------------------------------------------------------
# torchdyn
# ------------------------------------------------------------------------------------------------------------------------------
def _toy_field_torch():
    """A small smooth complex-valued, time-dependent vector field with the call signature of FlowModel's node_fn (t, x, args)."""
    import torch
    g = torch.Generator().manual_seed(3)
    A = 0.6 * torch.randn(12, 12, generator=g)
    c = torch.randn(12, generator=g)

    class F(torch.nn.Module):
        def forward(self, t, x, args=None):
            re, im = x.real, x.imag
            t = torch.as_tensor(t, dtype=torch.float32)
            return torch.complex(torch.tanh(re @ A.T + t * c) - 0.3 * im, torch.sin(im @ A + (1 - t) * c) + 0.2 * re)

    return F(), A.numpy(), c.numpy()


def _toy_field_numpy(A, c):
    def f(t, x):
        re, im = x.real.astype(np.float32), x.imag.astype(np.float32)
        t = np.float32(t)
        out_re = np.tanh(re @ A.T + t * c) - np.float32(0.3) * im
        out_im = np.sin(im @ A + (np.float32(1) - t) * c) + np.float32(0.2) * re
        return (out_re + 1j * out_im).astype(np.complex64)
    return f


def pin_torchdyn(report, write=True):
    import inspect

    import torch
    from torchdyn.core import NeuralODE

    from flowdec_amd.model import ADAPTIVE_DEFAULT_TOL
    from oracle import flowdec_oracle as O

    sig = inspect.signature(NeuralODE.__init__)
    d_atol, d_rtol = sig.parameters["atol"].default, sig.parameters["rtol"].default
    report["torchdyn.NeuralODE default atol/rtol"] = dict(package=[d_atol, d_rtol], flowdec_amd=ADAPTIVE_DEFAULT_TOL,
                                                         status="PINNED" if d_atol == d_rtol == ADAPTIVE_DEFAULT_TOL else "MISMATCH")
    field, A, c = _toy_field_torch()
    f_np = _toy_field_numpy(A, c)
    g = torch.Generator().manual_seed(4)
    x0 = torch.complex(torch.randn(5, 12, generator=g), torch.randn(5, 12, generator=g))
    golden = dict(A=A, c=c, x0=x0.numpy())
    # fixed-step drivers exactly as FlowModel.enhance builds them (model.py:503-515): NeuralODE(node_fn, solver=..., sensitivity='adjoint')
    for solver, N in (("euler", 6), ("midpoint", 3), ("euler", 50)):
        node = NeuralODE(field, solver=solver, sensitivity="adjoint")
        t_span = torch.linspace(0, 1, N + 1)
        with torch.no_grad():
            traj = node.trajectory(x0, t_span=t_span)
        ref = traj[-1].numpy()
        got = O.odeint_fixed(f_np, x0.numpy().astype(np.complex64), O.t_span_linspace(N), solver=solver)
        err = float(np.abs(got - ref).max() / np.abs(ref).max())
        report[f"torchdyn fixed-step {solver} N={N}"] = dict(max_rel_err=err, status="PINNED" if err < 2e-6 else "MISMATCH")
        golden[f"fixed_{solver}_{N}"] = ref
    # the repo's own Heun variants subclass torchdyn's solver template (sampling/solvers.py) -- they need /root/reference; skipped here
    # adaptive drivers at the package defaults and at 1e-5
    for method in ("dopri5", "tsit5"):
        for tol in (None, 1e-5):
            kw = {} if tol is None else dict(atol=tol, rtol=tol)
            node = NeuralODE(field, solver=method, sensitivity="adjoint", **kw)
            calls = [0]
            orig = field.forward

            def counted(t, x, args=None, _o=orig):
                calls[0] += 1
                return _o(t, x, args)
            field.forward = counted
            with torch.no_grad():
                traj = node.trajectory(x0, t_span=torch.linspace(0, 1, 5))
            field.forward = orig
            ref = traj[-1].numpy()
            t = d_atol if tol is None else tol
            got, nfe = O.odeint_adaptive(f_np, x0.numpy().astype(np.complex64), O.linspace_f32(0.0, 1.0, 5), method, atol=t, rtol=t)
            err = float(np.abs(got - ref).max() / np.abs(ref).max())
            ok = err < 50 * t and nfe == calls[0]
            report[f"torchdyn {method} tol={'default' if tol is None else tol}"] = dict(max_rel_err=err, nfe_package=calls[0], nfe_oracle=int(nfe),
                                                                                     status="PINNED" if ok else "MISMATCH")
            golden[f"{method}_{'default' if tol is None else 'tight'}"] = ref
            golden[f"{method}_{'default' if tol is None else 'tight'}_nfe"] = np.int64(calls[0])
    if write:
        np.savez_compressed(os.path.join(GOLDEN, "g_pin_torchdyn.npz"), **golden)


# ------------------------------------------------------------------------------------------------------------------------------
# descript-audio-codec
# ------------------------------------------------------------------------------------------------------------------------------
def pin_dac(report, write=True):
    import torch
    import dac as dac_pkg

    from oracle import ndac_oracle as NO

    cfg = dict(encoder_dim=16, encoder_rates=[2, 4, 5, 8], latent_dim=64, decoder_dim=96, decoder_rates=[8, 5, 4, 2], n_codebooks=4,
               codebook_size=64, codebook_dim=8, sample_rate=48000)
    torch.manual_seed(0)
    m = dac_pkg.DAC(**cfg).eval()
    with torch.no_grad():      # default init leaves snake alphas at 1 and weight-norm g = ||v||: perturb everything so that each term matters
        for p in m.parameters():
            p.add_(0.05 * torch.randn_like(p))
    sd = {k: v.detach().cpu().numpy() for k, v in m.state_dict().items()}
    ora = NO.DACOracle(sd, **cfg)
    g = torch.Generator().manual_seed(1)
    x = 0.3 * torch.randn(2, 1, 320 * 7 + 13, generator=g)
    with torch.no_grad():
        xp = m.preprocess(x, cfg["sample_rate"])
        z, codes, latents, _, _ = m.encode(xp, n_quantizers=3)
        zq, _, _ = m.quantizer.from_codes(codes)
        y = m.decode(zq)
    xo = ora.preprocess(x.numpy(), cfg["sample_rate"])
    zo, codes_o, lat_o, _, _ = ora.encode(xo, n_quantizers=3)
    zq_o, _, _ = ora.from_codes(codes.numpy())
    yo = ora.decode(zq.numpy())
    rel = lambda a, b: float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))
    mism = int((codes_o != codes.numpy()).sum())
    report["dac preprocess"] = dict(equal=bool(np.array_equal(xo, xp.numpy())), status="PINNED" if np.array_equal(xo, xp.numpy()) else "MISMATCH")
    report["dac encode: code indices"] = dict(mismatches=mism, of=int(codes.numel()), status="PINNED" if mism <= codes.numel() // 200 else "MISMATCH")
    report["dac encode: latents (first codebook)"] = dict(max_rel_err=rel(lat_o[:, :8], latents.numpy()[:, :8]),
                                                          status="PINNED" if rel(lat_o[:, :8], latents.numpy()[:, :8]) < 1e-4 else "MISMATCH")
    report["dac quantizer.from_codes"] = dict(max_rel_err=rel(zq_o, zq.numpy()), status="PINNED" if rel(zq_o, zq.numpy()) < 1e-5 else "MISMATCH")
    report["dac decode"] = dict(max_rel_err=rel(yo, y.numpy()), status="PINNED" if rel(yo, y.numpy()) < 1e-4 else "MISMATCH")
    if write:
        np.savez_compressed(os.path.join(GOLDEN, "g_pin_dac.npz"), x=x.numpy(), xp=xp.numpy(), codes=codes.numpy(), latents=latents.numpy(),
                            zq=zq.numpy(), y=y.numpy(), cfg=json.dumps(cfg), **{"sd/" + k: v for k, v in sd.items()})


def run(write=True):
    report = {}
    status = {}
    for name, mod, fn in (("torchdyn", "torchdyn", pin_torchdyn), ("descript-audio-codec", "dac", pin_dac)):
        if not have(mod):
            status[name] = "absent"
            continue
        try:
            fn(report, write)
            status[name] = "checked"
        except Exception as e:   # a package that imports but behaves differently from 1.0.x: say so, do not crash the other check
            status[name] = f"error: {type(e).__name__}: {e}"
    return status, report


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--no-write", action="store_true", help="compare only, do not write tests/golden/g_pin_*.npz")
    ap.add_argument("--report", default=os.path.join(ROOT, "profiles", "pin_third_party_report.json"))
    a = ap.parse_args()
    status, report = run(write=not a.no_write)
    out = dict(packages=status, items=report)
    print(json.dumps(out, indent=1))
    if any(s == "checked" for s in status.values()):
        with open(a.report, "w") as f:
            json.dump(out, f, indent=1)
    bad = [k for k, v in report.items() if v.get("status") != "PINNED"] + [k for k, v in status.items() if v.startswith("error")]
    sys.exit(1 if bad else 0)
