"""GPU tests of the validation loss (include/flowdec_hip.h "Validation loss"; flowdec_amd/loss.py): the three kernels at operator level,
the whole call against the reference's `_loss` (tests/golden/g33_valid_loss.npz, made by tests/golden/make_golden_loss.py), batch
independence, seeded == buffer, the drawn times against the NumPy Philox oracle, and the refusals.  Every model is the nf = 8 one."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import load_golden, rel_err
from oracle import flowdec_oracle as O
from noise_oracle import philox4x32_10
from test_hip_model import BF16_MEAN_FACTOR, BF16_PRED8, TOL_FWD

pytestmark = pytest.mark.gpu

F = 768
KINDS = {"flow": 0, "score": 1, "regression": 2}
FLOW_CASES = {"flow_scalar_sx0": ("scalar", 0.0), "flow_scalar_sx01": ("scalar", 0.1), "flow_curve_sx0": ("curve", 0.0), "flow_curve_sx01": ("curve", 0.1)}
_cache = {}


def lib_():
    from flowdec_amd import _lib
    return _lib, _lib.load()


def golden():
    if "g" not in _cache:
        _cache["g"] = load_golden("g33_valid_loss.npz")
    return _cache["g"]


def golden_noise(n_draws, Tp=64, B=2):
    """The draws of the fixture: O.seeded_noises(noise_seed) -> complex64 [n_draws, B, 1, F, Tp] on the GPU (made once, never modified)."""
    key = ("noise", n_draws)
    if key not in _cache:
        stream = O.seeded_noises(int(golden()["noise_seed"]), (B, 1, F, Tp))
        _cache[key] = torch.from_numpy(np.stack([next(stream) for _ in range(n_draws)])).cuda()
    return _cache[key]


def make_model(kind, prec, sigma="curve"):
    """nf = 8 model of the class `kind` on the fixture's seeded weights (seed 8, unscaled), cached per (kind, precision, sigma_y form)."""
    key = (kind, prec, sigma)
    if key not in _cache:
        import flowdec_amd
        g = golden()
        name = {"flow": "flowdec_75m", "score": "baseline_scoredec_75s", "regression": "baseline_regression_75s"}[kind]
        m = flowdec_amd.from_preset(name, precision=prec, nf=8)
        if kind == "score":
            m.sde = flowdec_amd.OUVESDE(*[float(v) for v in g["sde"]], N=30)
            m.t_eps = float(g["t_eps"])
        if kind == "flow":
            sy = torch.tensor(float(g["sigma_y_scalar"])) if sigma == "scalar" else torch.from_numpy(g["sigma_y_curve"])
            m.sigma_y = torch.nn.Parameter(sy, requires_grad=False)
        sd = O.random_state_dict(seed=int(g["weight_seed"]), nf=8)
        res = m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items() if k.startswith("backbone.")}, strict=False)
        assert not res.unexpected_keys and not [k for k in res.missing_keys if k.startswith("backbone.")]
        _cache[key] = m.cuda()
    return _cache[key]


def tau(prec):
    """The relative L2 error the nf = 8 forward pass is held to in tests/test_hip_model.py: TOL_FWD, and for bf16 the committed
    oracle-with-bf16-roundings prediction times its factor.  That prediction depends on the input and is committed for two inputs, neither
    of them this fixture's: the larger of the two is taken."""
    return BF16_MEAN_FACTOR * max(BF16_PRED8["forward_rel_l2"].values()) if prec == "bf16" else TOL_FWD[prec]


def sums_bound(prec, sums_ref, vnorm2):
    """V = V_ref + e with ||e|| <= tau ||V_ref||:  | sum |V - U|^2 - sum |V_ref - U|^2 | <= 2 tau ||V_ref|| ||V_ref - U|| + tau^2 ||V_ref||^2."""
    t = tau(prec)
    return 2 * t * np.sqrt(vnorm2) * np.sqrt(sums_ref) + t * t * vnorm2


def sqerr(kind, V, U, std=None):
    _lib, lib = lib_()
    B, _, Fq, Tp = V.shape
    nws = int(lib.fd_loss_sqerr_workspace_bytes(B, Fq, Tp))
    assert nws > 0
    ws = torch.empty(nws, dtype=torch.uint8, device="cuda")
    sums = torch.empty(B, dtype=torch.float64, device="cuda")
    bad = torch.empty(B, dtype=torch.int64, device="cuda")
    _lib.check(lib.fd_loss_sqerr(KINDS[kind], _lib.ptr(torch.view_as_real(V)), _lib.ptr(torch.view_as_real(U)), _lib.ptr(std), _lib.ptr(sums), _lib.ptr(bad),
                                 B, Fq, Tp, _lib.ptr(ws), nws, _lib.stream()))
    return sums.cpu().numpy(), bad.cpu().numpy()


# ---- 1. the reduction, exact ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Tp", [64, 128])
@pytest.mark.parametrize("kind", ["flow", "score", "regression"])
def test_sqerr_exact_on_integers(kind, Tp):
    """Integer-valued V and target with |.| <= 64 (std a power of two in score mode): every float32 difference, every product and every
    float64 partial sum is an exact integer, so the result equals NumPy's int64 sums whatever the order.  A NaN planted in clip 1 is
    counted there and leaves the other clips' sums unchanged."""
    rng = np.random.default_rng(100 + Tp)
    B = 3
    vi, ui = rng.integers(-64, 65, (2, B, 1, F, Tp, 2))
    V = torch.view_as_complex(torch.from_numpy(vi.astype(np.float32))).cuda()
    U = torch.view_as_complex(torch.from_numpy(ui.astype(np.float32))).cuda()
    std = torch.tensor([0.5, 2.0, 0.125], device="cuda") if kind == "score" else None
    want = ((vi - ui) ** 2).reshape(B, -1).sum(axis=1)
    sums, bad = sqerr(kind, V, U, std)
    assert sums.dtype == np.float64 and (sums == want.astype(np.float64)).all(), (sums, want)
    assert bad.tolist() == [0, 0, 0]
    Vn = V.clone()
    Vn[1, 0, 123, Tp - 1] = complex(float("nan"), 1.0)
    sums_n, bad_n = sqerr(kind, Vn, U, std)
    assert bad_n.tolist() == [0, 1, 0]
    assert sums_n[0] == want[0] and sums_n[2] == want[2] and np.isnan(sums_n[1])


# ---- 2. the state kernel -------------------------------------------------------------------------------------------------------------------
def loss_state(kind_cfg, Y, X, t, noise, seeds, sigma, want_ys=False):
    _lib, lib = lib_()
    B, _, Fq, Tp = Y.shape
    xt, tg = torch.empty_like(Y), torch.empty_like(Y)
    ys = torch.empty_like(Y) if want_ys else None
    std = torch.empty(B, dtype=torch.float32, device="cuda")
    r = lambda z: None if z is None else _lib.ptr(torch.view_as_real(z))
    _lib.check(lib.fd_loss_state(C.byref(kind_cfg), r(Y), r(X), _lib.ptr(t), r(noise), _lib.ptr(seeds), _lib.ptr(sigma), 0 if sigma is None else sigma.numel(),
                                 r(xt), r(tg), _lib.ptr(std), r(ys), B, Fq, Tp, _lib.stream()))
    return xt, tg, std, ys


def test_state_kernel_vs_reference_and_ode_x0():
    _lib, lib = lib_()
    g = golden()
    name = str(g["state_case"])
    noise = golden_noise(2)
    t = torch.from_numpy(g[name + "_t"]).cuda()
    sigma = torch.from_numpy(g["sigma_y_curve"]).reshape(-1).double().cuda()
    cfg = _lib.FdLossConfig(kind=0, sigma_x=float(np.float32(FLOW_CASES[name][1])))
    # (a) on the reference's OWN spectrograms of clip 1 (every 4th frequency row, all frames: the arithmetic is elementwise), so that
    # only the state arithmetic is compared: relative L2 <= 1e-6, the float32-rounding bound of the suite's elementwise comparisons
    fs = int(g["state_fstride"])
    xt, ut, _, _ = loss_state(cfg, torch.from_numpy(g["state_Y"]).cuda(), torch.from_numpy(g["state_X"]).cuda(), t[1:2].contiguous(),
                              noise[:, 1:2, :, ::fs].contiguous(), None, sigma[::fs].contiguous())
    e_xt, e_ut = rel_err(xt.cpu().numpy(), g["state_Xt"]), rel_err(ut.cpu().numpy(), g["state_Ut"])
    print(f"state kernel vs reference: Xt {e_xt:.3e}  Ut {e_ut:.3e}")
    assert e_xt <= 1e-6 and e_ut <= 1e-6
    # (b) Ys is the initial state of the ODE solve on the same noise plane, bit for bit (full planes, this library's front end)
    m = make_model("flow", "fp32", "curve")
    y, x = torch.from_numpy(g["y"]), torch.from_numpy(g["x"])
    Y, X, _ = m._preprocess(y, x=x)
    _, _, _, ys = loss_state(cfg, Y, X, t, noise, None, sigma, want_ys=True)
    traj, _ = m.enhance(y, N=1, solver="euler", return_traj=True, noise=noise[0], use_graph=False)
    assert torch.equal(torch.view_as_real(ys), torch.view_as_real(traj[0].reshape(ys.shape)))


# ---- 3. against the reference --------------------------------------------------------------------------------------------------------------
def _check_case(prec, kind, name, model, n_draws):
    g = golden()
    kw = {} if kind == "regression" else dict(noise=golden_noise(n_draws), t=torch.from_numpy(g[name + "_t"]))
    loss = model.valid_loss(torch.from_numpy(g["x"]), torch.from_numpy(g["y"]), **kw)
    info = model.last_loss_info
    sums_ref, vn2 = g[name + "_sums"], g[name + "_vnorm2"]
    bound = sums_bound(prec, sums_ref, vn2)
    diff = np.abs(info["sums"] - sums_ref)
    print(f"{name}[{prec}]: loss {loss:.6g} ref {float(g[name + '_loss']):.6g}  |sums - ref| / bound {diff / bound}")
    assert (info["bad"] == 0).all()
    assert (diff <= bound).all(), (name, prec, diff, bound)
    # the reduced loss: the same bound pushed through the reference's reduction, plus the float32 rounding of the reference's own
    # mean over 49152 values (1e-5 relative is generous for a pairwise float32 sum)
    n_bins = F * 64
    scale = {"flow": 1.0 / (2 * n_bins), "score": 0.5 / 2, "regression": 1.0 / (2 * n_bins)}[kind]
    ref = float(g[name + "_loss"])
    assert abs(loss - ref) <= scale * bound.sum() + 1e-5 * abs(ref), (name, prec, loss, ref)


@pytest.mark.parametrize("prec", ["fp32", "bf16x3", "mixed", "bf16"])
def test_valid_loss_vs_reference(prec):
    for name, (sy, sx) in FLOW_CASES.items():
        m = make_model("flow", prec, sy)
        m.sigma_x.data = torch.tensor(sx, device=m.sigma_x.device)
        _check_case(prec, "flow", name, m, 2 if sx else 1)
    _check_case(prec, "score", "score", make_model("score", prec), 1)
    _check_case(prec, "regression", "regression", make_model("regression", prec), 0)


# ---- 4. independence -----------------------------------------------------------------------------------------------------------------------
def _clips():
    if "clips" not in _cache:
        rng = np.random.default_rng(44)
        out = []
        for i, n in enumerate((12000, 9217, 12000, 25000)):
            x = (0.1 * (1 + i) * rng.standard_normal(n)).astype(np.float32)
            out.append((torch.from_numpy(x), torch.from_numpy((x + 0.02 * rng.standard_normal(n)).astype(np.float32))))
        _cache["clips"] = out
    return _cache["clips"]


@pytest.mark.parametrize("kind", ["flow", "score", "regression"])
def test_clip_is_independent_of_its_batch(kind):
    """Loss, time and normfac of a clip are bit-identical alone, in a batch, with the batch order permuted, and across two T_pad buckets."""
    m = make_model(kind, "bf16")
    if kind == "flow":
        m.sigma_x.data = torch.tensor(0.1, device=m.sigma_x.device)
    clips = _clips()
    seeds = [11, 2 ** 63 + 5, 12345678901234567, 77]
    rnd = kind != "regression"

    def run(idx, **kw):
        kw = dict(kw, seeds=[seeds[i] for i in idx]) if rnd else kw
        v = m.valid_loss_batch([clips[i][0] for i in idx], [clips[i][1] for i in idx], reduce="none", **kw)
        info = m.last_loss_info
        return v, (info["t"].numpy() if rnd else np.zeros(len(idx), np.float32)), info["normfac"].numpy()

    alone = [run([i]) for i in range(4)]
    for order in ([0, 1, 2], [2, 0, 1], [3, 1, 0, 2], [1, 3]):
        v, t, nf = run(order, max_batch=3)
        for k, i in enumerate(order):
            assert v[k] == alone[i][0][0] and t[k] == alone[i][1][0] and nf[k] == alone[i][2][0], (kind, order, k)
    # the one-length form (no lengths array) on the 12000-sample clip
    one = m.valid_loss(clips[0][0], clips[0][1], reduce="none", **(dict(seed=[seeds[0]]) if rnd else {}))
    assert one[0] == alone[0][0][0]
    assert np.isfinite([a[0][0] for a in alone]).all()


# ---- 5. seeded == buffer -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["flow", "score"])
def test_seeded_equals_buffer(kind):
    from flowdec_amd import loss as fd_loss, noise as fd_noise
    m = make_model(kind, "bf16")
    if kind == "flow":
        m.sigma_x.data = torch.tensor(0.1, device=m.sigma_x.device)
    g = golden()
    x, y = torch.from_numpy(g["x"]), torch.from_numpy(g["y"])
    s = 20261019
    a, ta = m.valid_loss(x, y, seed=s, reduce="none", return_t=True)
    seeds = fd_noise.seeds_to_tensor(s, 2, "cuda")
    planes = fd_noise.noise_fill(seeds, F, 64, draw0=0, n_draws=2 if kind == "flow" else 1)
    t = fd_loss.loss_times(seeds, *fd_loss.time_range(m, kind))
    b, tb = m.valid_loss(x, y, noise=planes, t=t, reduce="none", return_t=True)
    assert (a == b).all() and torch.equal(ta, tb) and np.isfinite(a).all()


# ---- 6. the drawn times --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lo,hi", [(0.0, 1.0), (0.03, 1.0)])
def test_times_match_the_philox_oracle(lo, hi):
    from flowdec_amd import loss as fd_loss, noise as fd_noise
    vals = [fd_noise.clip_seed(7, i) for i in range(62)] + [0, 2 ** 64 - 1]
    t = fd_loss.loss_times(fd_noise.seeds_to_tensor(vals, 64, "cuda"), lo, hi).cpu().numpy()
    lo32, hi32 = np.float32(lo), np.float32(hi)
    want = np.empty(64, np.float32)
    for i, s in enumerate(vals):
        r0 = int(philox4x32_10(0, 0, 0, 1, s & 0xFFFFFFFF, s >> 32)[0])
        u = np.float32((r0 >> 8) * 2.0 ** -24)
        want[i] = np.float32(u * np.float32(hi32 - lo32)) + lo32
    assert (t == want).all()
    assert (t >= lo32).all() and (t < hi32).all()
    assert len(set(t.tolist())) > 60


# ---- 7. refusals ---------------------------------------------------------------------------------------------------------------------------
def test_refusals():
    import types
    import flowdec_amd
    _lib, lib = lib_()
    g = golden()
    m = make_model("flow", "bf16")
    x, y = torch.from_numpy(g["x"]), torch.from_numpy(g["y"])
    m.last_loss_info = None

    def refused(exc, **attrs):
        old = {k: m.__dict__.get(k, None) for k in attrs}
        had = {k: k in m.__dict__ for k in attrs}
        try:
            for k, v in attrs.items():
                object.__setattr__(m, k, v)
            with pytest.raises(exc):
                m.valid_loss(x, y, seed=1)
        finally:
            for k in attrs:
                if had[k]:
                    object.__setattr__(m, k, old[k])
                else:
                    object.__delattr__(m, k)
    refused(NotImplementedError, flow_matcher=types.SimpleNamespace(sigma=0.1))
    refused(NotImplementedError, error_weighting=torch.ones(F, 1))
    with pytest.raises(NotImplementedError):
        m.valid_loss(x, y, seed=1, comp_eps=1e-3)
    with pytest.raises(RuntimeError):
        m.valid_loss(x, y[:, :, :-1], seed=1)
    # a callable sigma_x (model.py:408-413) is kept by the constructor and refused by the loss
    cpu_model = flowdec_amd.from_preset("flowdec_75m", precision="bf16", nf=8)
    with pytest.raises(RuntimeError, match="GPU"):
        cpu_model.valid_loss(x, y, seed=1)
    fm = flowdec_amd.FlowModel(backbone=cpu_model.backbone, feature_extractor=cpu_model.feature_extractor, sampling_rate=48000,
                               sigma_x=lambda v: 0.1 * torch.ones_like(v.real), sigma_y=0.66)
    with pytest.raises(NotImplementedError, match="sigma_x"):
        fm.valid_loss(x, y, seed=1)
    assert m.last_loss_info is None                     # nothing ran
    # through the ABI: a NULL x is FD_EINVAL and the message names the argument; nothing is written
    h = m._sync_native()
    cfg = _lib.FdLossConfig(kind=0)
    need = int(lib.fd_valid_loss_workspace_bytes(h, 2, 12000))
    assert need > 0 and lib.fd_valid_loss_workspace_bytes(h, 257, 12000) == 0 and lib.fd_valid_loss_workspace_bytes(h, 2, 700) == 0
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    yd = y.reshape(2, -1).cuda()
    seeds = torch.tensor([1, 2], dtype=torch.int64, device="cuda")
    sums = torch.full((2,), -1.0, dtype=torch.float64, device="cuda")
    bad = torch.zeros(2, dtype=torch.int64, device="cuda")
    nf = torch.zeros(2, device="cuda")
    args = lambda xp, nbytes=need, sd=_lib.ptr(seeds): (h, C.byref(cfg), xp, _lib.ptr(yd), None, None, sd, None, _lib.ptr(sums), _lib.ptr(bad), _lib.ptr(nf),
                                                          2, 12000, _lib.ptr(ws), nbytes, _lib.stream())
    assert lib.fd_valid_loss(*args(None)) == -1 and b"null x" in lib.fd_last_error()
    assert lib.fd_valid_loss(*args(_lib.ptr(yd), nbytes=need - 1024)) == -1 and b"workspace" in lib.fd_last_error()
    assert lib.fd_valid_loss(*args(_lib.ptr(yd), sd=None)) == -1 and b"noise and seeds" in lib.fd_last_error()
    torch.cuda.synchronize()
    assert (sums == -1.0).all() and (nf == 0).all()


# ---- 8. the command line, end to end -------------------------------------------------------------------------------------------------------
def test_cli_end_to_end_is_independent_of_the_batch_size(tmp_path):
    """loss_cli on a saved nf = 8 checkpoint and four wav pairs of three lengths (--no-crop: two T_pad buckets): the per-pair values and
    the loss are the same bits at --batch 1 and --batch 3, and equal the model's own valid_loss_batch with seeds clip_seed(seed, i)."""
    import io
    from flowdec_amd import enhance_cli, loss_cli
    from test_cli import synthetic_ckpt
    torch.save(synthetic_ckpt(), tmp_path / "m.ckpt")
    rng = np.random.default_rng(5)
    lines, xs, ys = [], [], []
    for i, n in enumerate((12000, 25000, 9217, 12000)):
        x = (0.1 * rng.standard_normal(n)).astype(np.float32)
        y = (x + 0.02 * rng.standard_normal(n)).astype(np.float32)
        enhance_cli.save_wav(str(tmp_path / f"x{i}.wav"), torch.from_numpy(x)[None], 48000)
        enhance_cli.save_wav(str(tmp_path / f"y{i}.wav"), torch.from_numpy(y)[None], 48000)
        lines.append(f"{tmp_path / f'x{i}.wav'} ---> {tmp_path / f'y{i}.wav'}")
    (tmp_path / "pairs.txt").write_text("\n".join(lines) + "\n")
    base = ["--ckpt", str(tmp_path / "m.ckpt"), "--pairs-file", str(tmp_path / "pairs.txt"), "--no-crop", "--seed", "9"]
    a = loss_cli.run(base + ["--batch", "1"], out=io.StringIO())
    b = loss_cli.run(base + ["--batch", "3", "--out", str(tmp_path / "l.csv")], out=io.StringIO())
    assert a.kind == "flow" and np.isfinite(a.per_pair).all() and a.loss == b.loss
    assert np.array_equal(a.per_pair, b.per_pair) and np.array_equal(a.t, b.t) and len(set(a.t.tolist())) == 4
    assert len((tmp_path / "l.csv").read_text().strip().splitlines()) == 5
    m = enhance_cli.load_from_checkpoint(str(tmp_path / "m.ckpt"), map_location="cuda", precision="bf16")
    xs = [enhance_cli.load_wav(str(tmp_path / f"x{i}.wav"))[0][0] for i in range(4)]
    ys = [enhance_cli.load_wav(str(tmp_path / f"y{i}.wav"))[0][0] for i in range(4)]
    direct = m.valid_loss_batch(xs, ys, seeds=9, reduce="none", max_batch=4)
    assert np.array_equal(direct, a.per_pair)
