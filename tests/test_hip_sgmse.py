"""The SGMSE-style backbone on the GPU: the attention block alone (fd_attn_block) against the reference (G26) and a float64 NumPy
restatement, whole forwards (G27 nf 8, G28 nf 128) and enhance (G29) against the reference, the bf16 mode against its derived
prediction (G30), and the bit-identity guarantees (repeat, graph == eager, clip in a batch == alone, ragged batch == one by one)."""
import ctypes as C
import importlib.util as ilu
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, load_golden, rel_err
from test_hip_ops import check, report

pytestmark = pytest.mark.gpu

PRED = json.load(open(os.path.join(GOLDEN, "g30_sgmse_bf16_prediction.json")))["rel_l2"]
TOL_FWD = {"fp32": 2e-4, "bf16x3": 2e-4}      # TOL_FWD_FULL of test_hip_model.py; "mixed" rounds a subset of the bf16 mode's points:
                                               # 1.3 x the bf16 prediction of that golden
TOL_WAVE = {"fp32": 5e-4, "bf16x3": 5e-4}
_spec = ilu.spec_from_file_location("_mg_sgmse", os.path.join(GOLDEN, "make_golden_sgmse.py"))
GEN = ilu.module_from_spec(_spec)
_spec.loader.exec_module(GEN)

_cache = {}


def make_model(nf, precision, preset="flow_model_sgmse", seed=None):
    key = (nf, precision, preset)
    if key not in _cache:
        import flowdec_amd
        m = flowdec_amd.from_preset(preset, precision=precision, nf=nf)
        shapes = {"backbone." + k: list(v.shape) for k, v in m.backbone.state_dict().items()}
        sd = GEN.random_params(nf if seed is None else seed, shapes)
        if preset == "score_model_sgmse":
            sd["backbone.output_layer.weight"] = (sd["backbone.output_layer.weight"] * np.float32(GEN.SCORE_OUT_SCALE)).astype(np.float32)
        missing, unexpected = m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=False)
        assert not unexpected and not [k for k in missing if k.startswith("backbone.")]
        _cache[key] = m.cuda()
    return _cache[key]


def pinned(a, key_sum):
    """An input re-derived by the generator, checked against the checksum the fixture stores."""
    np.testing.assert_allclose(GEN.checksum(a), key_sum, rtol=1e-9, atol=1e-6)
    return a


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---------------------------------------------------------------------------------------------------------------------
# the attention block alone
# ---------------------------------------------------------------------------------------------------------------------
def attn_ref64(x, p):
    """AttnBlockpp (skip_rescale) in float64 on NHWC x [B, H, W, C]."""
    B, H, W, Cc = x.shape
    xx = x.reshape(B, H * W, Cc).astype(np.float64)
    G = min(Cc // 4, 32)
    xg = xx.reshape(B, H * W, G, Cc // G)
    mean = xg.mean(axis=(1, 3), keepdims=True)
    var = xg.var(axis=(1, 3), keepdims=True)
    h = ((xg - mean) / np.sqrt(var + 1e-6)).reshape(B, H * W, Cc) * p["GroupNorm_0.weight"] + p["GroupNorm_0.bias"]
    q, k, v = (h @ p[f"NIN_{i}.W"].astype(np.float64) + p[f"NIN_{i}.b"] for i in range(3))
    s = q @ k.transpose(0, 2, 1) * Cc ** -0.5
    s -= s.max(-1, keepdims=True)
    w = np.exp(s)
    w /= w.sum(-1, keepdims=True)
    o = (w @ v) @ p["NIN_3.W"].astype(np.float64) + p["NIN_3.b"]
    return ((xx + o) / np.sqrt(2.0)).reshape(B, H, W, Cc)


def run_attn(x_nhwc, p, dtype, stats=False):
    from flowdec_amd import _lib as L
    lib = L.load()
    B, H, W, Cc = x_nhwc.shape
    tdt = torch.bfloat16 if dtype == "bf16" else torch.float32
    fdt = L.FD_BF16 if dtype == "bf16" else L.FD_F32
    dev = {k: cu(v.astype(np.float32)) for k, v in p.items()}
    wqkv = torch.cat([dev[f"NIN_{i}.W"] for i in range(3)], dim=1).contiguous()
    bqkv = torch.cat([dev[f"NIN_{i}.b"] for i in range(3)]).contiguous()
    d = L.FdAttnDesc(Cc, L.ptr(dev["GroupNorm_0.weight"]), L.ptr(dev["GroupNorm_0.bias"]), L.ptr(wqkv), L.ptr(bqkv), L.ptr(dev["NIN_3.W"]),
                     L.ptr(dev["NIN_3.b"]))
    x = cu(x_nhwc).to(tdt).contiguous()
    out = torch.empty_like(x)
    need = lib.fd_attn_block_workspace_bytes(C.byref(d), B, H, W, fdt)
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    st = torch.zeros(B, (H * W + 15) // 16, Cc, 2, device="cuda") if stats else None
    L.check(lib.fd_attn_block(C.byref(d), L.ptr(x), L.ptr(out), L.ptr(st) if stats else None, B, H, W, fdt, L.ptr(ws), ws.numel(), L.stream()))
    torch.cuda.synchronize()
    return x.float().cpu().numpy(), out.float().cpu().numpy(), (st.cpu().numpy() if stats else None)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_attn_block_vs_reference(dtype):
    g = load_golden("g26_attn_block.npz")
    for big in (False, True):
        p = GEN.attn_params(256, big)
        for (B, H, W) in GEN.ATTN_SHAPES if not big else GEN.ATTN_SHAPES[2:]:
            nm = f"{'big_' if big else ''}{B}x{H}x{W}"
            x = pinned(GEN.attn_input(B, H, W, big), g[nm + "_x_sum"]).transpose(0, 2, 3, 1)
            xs, out, _ = run_attn(x, p, dtype)
            # the reference output is stored whole (small cases) or as the generator's regular sample of its NCHW layout
            full = nm + "_out" in g.files
            ref = g[nm + "_out"].transpose(0, 2, 3, 1) if full else g[nm + "_out_s"]
            pick = (lambda a: a) if full else (lambda a: GEN.sample(a.transpose(0, 3, 1, 2)))
            if dtype == "fp32":   # K = 256 sums and one softmax in f32 (u = 6e-8)
                check(f"attn_block_g26[fp32][{nm}]", pick(out), ref, 2e-5)
            else:
                # against the exact block on the stored (rounded) input: only the output rounding (u = 3.9e-3) remains
                exact = attn_ref64(xs, p)
                check(f"attn_block_f64_on_stored_input[{nm}]", out, exact, 3e-3)
                # against the reference: plus what the input rounding alone does to the exact block (amplified by large logits)
                check(f"attn_block_g26[bf16][{nm}]", pick(out), ref, 3e-3 + rel_err(pick(exact), ref))


@pytest.mark.parametrize("Cc", [16, 64, 256])
@pytest.mark.parametrize("scale", [1.0, 8.0])
def test_attn_block_vs_float64(Cc, scale):
    """Several seeds, shapes and logit scales (x 64 at scale 8: a softmax without max subtraction overflows there)."""
    for seed, (B, H, W) in enumerate(((1, 12, 1), (2, 12, 3), (1, 12, 21), (1, 24, 9))):
        rng = np.random.default_rng(100 * Cc + seed)
        shapes = {"GroupNorm_0.weight": (Cc,), "GroupNorm_0.bias": (Cc,)}
        for i in range(4):
            shapes[f"NIN_{i}.W"] = (Cc, Cc); shapes[f"NIN_{i}.b"] = (Cc,)
        p = GEN.random_params(seed + 7 * Cc, shapes, std=0.3)
        p["NIN_0.W"] = (p["NIN_0.W"] * np.float32(scale)).astype(np.float32)
        p["NIN_1.W"] = (p["NIN_1.W"] * np.float32(scale)).astype(np.float32)
        x = (rng.standard_normal((B, H, W, Cc)) * 2.0 - 0.5).astype(np.float32)
        for dtype in ("fp32", "bf16"):
            xs, out, st = run_attn(x, p, dtype, stats=True)
            ref = attn_ref64(xs, p)
            assert np.isfinite(out).all()
            check(f"attn_block_f64[C{Cc} x{scale} {B}x{H}x{W}][{dtype}]", out, ref, (4e-5 * scale if dtype == "fp32" else 3e-3))
            # GroupNorm partial sums of the stored output, 16 positions per tile
            N = H * W
            o = out.reshape(B, N, Cc).astype(np.float64)
            pad = np.zeros((B, st.shape[1] * 16 - N, Cc))
            o = np.concatenate([o, pad], axis=1).reshape(B, st.shape[1], 16, Cc)
            np.testing.assert_allclose(st[..., 0], o.sum(2), rtol=1e-4, atol=1e-3)
            np.testing.assert_allclose(st[..., 1], (o ** 2).sum(2), rtol=1e-4, atol=1e-3)


def test_attn_block_batch_invariant():
    p = GEN.attn_params(256)
    rng = np.random.default_rng(5)
    x = rng.standard_normal((5, 12, 7, 256)).astype(np.float32)
    for dtype in ("fp32", "bf16"):
        _, out, _ = run_attn(x, p, dtype)
        _, out2, _ = run_attn(x, p, dtype)
        assert np.array_equal(out, out2)
        for b in (0, 3):
            _, one, _ = run_attn(x[b:b + 1], p, dtype)
            assert np.array_equal(one[0], out[b])


# ---------------------------------------------------------------------------------------------------------------------
# whole network
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nf,golden", [(8, "g27_ncsnpp_sgmse_nf8.npz"), (128, "g28_ncsnpp_sgmse_nf128.npz")])
@pytest.mark.parametrize("prec", ["fp32", "bf16x3", "mixed", "bf16"])
def test_sgmse_forward_golden(nf, golden, prec):
    g = load_golden(golden)
    m = make_model(nf, prec)
    x, y = GEN.forward_inputs(nf)
    pinned(x, g["x_sum"]); pinned(y, g["y_sum"])
    for key, t in (("out_t025", [0.25]), ("out_t01_09", [0.1, 0.9])):
        full = m.backbone(cu(x), cu(y), torch.tensor(t, device="cuda")).cpu().numpy()
        assert np.isfinite(full).all()
        out = GEN.sample(full)   # the stored regular sample of the reference output
        key = key + "_s"
        if prec == "bf16":
            pred = PRED[f"{golden[:3]}_{key[:-2]}"]
            e = rel_err(out, g[key])
            report(f"sgmse_nf{nf}_bf16_vs_prediction[{key}]", e / pred, 1.3)
            assert 0.3 * pred < e < 1.3 * pred, (e, pred)
        else:
            tol = 1.3 * PRED[f"{golden[:3]}_{key[:-2]}"] if prec == "mixed" else TOL_FWD[prec]
            check(f"sgmse_nf{nf}[{prec}][{key}]", out, g[key], tol)


@pytest.mark.parametrize("prec", ["fp32", "bf16x3", "bf16"])
def test_sgmse_enhance_golden(prec):
    g = load_golden("g29_enhance_sgmse_nf128.npz")
    m = make_model(128, prec)
    y, noise = GEN.enhance_inputs()
    pinned(y, g["y_sum"]); pinned(noise, g["noise_sum"])
    for solver, N in (("euler", 6), ("midpoint", 3)):
        x = GEN.sample(m.enhance(torch.from_numpy(y), N=N, solver=solver, noise=torch.from_numpy(noise)).numpy())
        ref = g[f"{solver}_N{N}_s"]
        if prec == "bf16":
            pred = PRED[f"g29_{solver}_N{N}"]
            e = rel_err(x, ref)
            report(f"sgmse_enhance_bf16_vs_prediction[{solver}_N{N}]", e / pred, 1.6)
            assert 0.3 * pred < e < 1.6 * pred, (e, pred)
        else:
            check(f"sgmse_enhance[{prec}][{solver}_N{N}]", x, ref, TOL_WAVE[prec])


@pytest.mark.parametrize("prec", ["fp32", "bf16x3"])
def test_sgmse_score_sampler_golden(prec):
    from oracle import flowdec_oracle as O
    g = load_golden("g29_enhance_sgmse_nf128.npz")
    m = make_model(8, prec, preset="score_model_sgmse")
    y = pinned(GEN.score_input(), g["score_y_sum"])
    Tp = O.padded_frames(O.num_frames(y.shape[-1]))
    n = m.num_draws(3, "reverse_diffusion", "ald", 1)
    stream = O.seeded_noises(int(g["score_noise_seed"]), (2, 1, 768, Tp))
    noise = np.stack([next(stream) for _ in range(n)])
    x = m.enhance(torch.from_numpy(y), N=3, predictor="reverse_diffusion", corrector="ald", corrector_steps=1, snr=0.5,
                  noise=torch.from_numpy(noise)).numpy()
    check(f"sgmse_score_pc[{prec}]", x, g["score_rd_ald_N3"], TOL_WAVE[prec])


# ---------------------------------------------------------------------------------------------------------------------
# bit identity
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_sgmse_bit_identity(prec):
    from flowdec_amd import ops
    m = make_model(128, prec)
    rng = np.random.default_rng(77)
    # T_pad = 64: the bottleneck image is 12 x 1
    x = (rng.standard_normal((8, 1, 768, 64, 2)) / np.sqrt(2)).astype(np.float32).view(np.complex64)[..., 0]
    y = (rng.standard_normal((8, 1, 768, 64, 2)) / np.sqrt(2)).astype(np.float32).view(np.complex64)[..., 0]
    t = torch.tensor([0.4], device="cuda")
    before = ops.conv_kernel_counts()
    a = m.backbone(cu(x), cu(y), t)
    after = ops.conv_kernel_counts()
    report(f"sgmse_conv_launches_per_forward[{prec}]", float(sum(after.values()) - sum(before.values())), 1e9)
    print({k: after[k] - before[k] for k in after if after[k] != before[k]})
    assert sum(after.values()) > sum(before.values())
    b = m.backbone(cu(x), cu(y), t)
    assert torch.equal(torch.view_as_real(a), torch.view_as_real(b))
    for i in (0, 5):   # a clip inside a batch of 8 == the clip alone
        one = m.backbone(cu(x[i:i + 1]), cu(y[i:i + 1]), t)
        assert torch.equal(torch.view_as_real(one[0]), torch.view_as_real(a[i]))
    # graph == eager (the second identical call replays a captured graph), and ragged batch == one by one in one T_pad bucket
    lens = (40000, 47000, 48000)     # T_pad 128 for all three
    clips = [(0.1 * rng.standard_normal(L)).astype(np.float32) for L in lens]
    noises = [(rng.standard_normal((1, 1, 768, 128, 2)) / np.sqrt(2)).astype(np.float32).view(np.complex64)[..., 0] for _ in lens]
    eager = [m.enhance(torch.from_numpy(c), N=2, solver="midpoint", noise=torch.from_numpy(n), use_graph=False) for c, n in zip(clips, noises)]
    for _ in range(2):
        g0 = m.enhance(torch.from_numpy(clips[0]), N=2, solver="midpoint", noise=torch.from_numpy(noises[0]), use_graph=True)
        assert torch.equal(g0, eager[0])
    batch = m.enhance_batch([torch.from_numpy(c) for c in clips], N=2, solver="midpoint", noise=[torch.from_numpy(n) for n in noises])
    for o, e in zip(batch, eager):
        assert torch.equal(o, e)
