"""CPU-only tests: the C ABI exports every declared symbol, the host-side mirror of the reference API behaves like
the reference (state_dict layout, presets, errors), and the multi-GPU batch sharding is correct (gloo, world size 2)."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT, load_golden


def header_functions():
    src = open(os.path.join(ROOT, "include", "flowdec_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(fd_[a-z0-9_]+)\s*\(", src)))


def test_abi_exports_every_declared_symbol():
    import __graft_entry__ as g
    g.build()                                   # compiles for gfx950 with hipcc (no GPU needed) and loads the library
    from flowdec_amd import _lib
    lib = _lib.load()
    names = header_functions()
    assert len(names) >= 30
    for n in names:
        assert hasattr(lib, n), f"{n} declared in include/flowdec_hip.h but not exported"
        assert n in _lib.SIGNATURES, f"{n} has no ctypes signature in flowdec_amd/_lib.py"
    assert set(_lib.SIGNATURES) <= set(names)
    assert lib.fd_version() >= 100
    # pure host helpers of the ABI (no GPU needed): frame bookkeeping is integer exact
    assert [lib.fd_num_frames(L, 384) for L in (4800, 48000, 96000, 192000)] == [13, 126, 251, 501]
    assert [lib.fd_padded_frames(t) for t in (1, 64, 65, 126, 251, 501)] == [64, 64, 128, 128, 256, 512]
    assert lib.fd_upfirdn2d_out_size(768, 1, 2, 1, 1, 4) == 384 and lib.fd_upfirdn2d_out_size(96, 2, 1, 2, 1, 4) == 192
    assert lib.fd_conv_cout_pad(4) == 32 and lib.fd_conv_cout_pad(128) == 128 and lib.fd_conv_cout_pad(256) == 256
    assert lib.fd_conv_stats_tiles(768, 256) == 48 * 16
    # the kernel-dispatch counters: one per FD_CONV_KERNEL_* slot, written to host memory
    import ctypes as C
    assert lib.fd_conv_kernel_counts(None, 0) == len(_lib.CONV_KERNELS) == 9
    buf = (C.c_longlong * 12)(*([-1] * 12))
    assert lib.fd_conv_kernel_counts(buf, 12) == 9
    assert min(buf[:9]) >= 0 and list(buf)[9:] == [-1] * 3          # writes min(n, FD_CONV_KERNEL_COUNT) slots
    buf = (C.c_longlong * 2)(-1, -1)
    assert lib.fd_conv_kernel_counts(buf, 1) == 9 and buf[0] >= 0 and buf[1] == -1


def test_model_create_validates_arguments():
    import ctypes as C
    from flowdec_amd import _lib
    lib = _lib.load()
    cfg = _lib.FdModelConfig()
    cfg.nf, cfg.num_levels, cfg.num_res_blocks, cfg.n_fft, cfg.hop, cfg.act_dtype = 64, 4, 1, 1534, 384, 1
    for i, c in enumerate((4, 4, 4, 2)):
        cfg.ch_mult[i] = c
    h = C.c_void_p()
    assert lib.fd_model_create(C.byref(cfg), C.byref(h)) == 0
    n = lib.fd_model_num_params(h)
    names = {}
    for i in range(n):
        name, nd, shp = C.c_char_p(), C.c_int(), (C.c_int * 4)()
        assert lib.fd_model_param_info(h, i, C.byref(name), C.byref(nd), C.byref(shp)) == 0
        names[name.value.decode()] = [shp[j] for j in range(nd.value)]
    with open(os.path.join(GOLDEN, "state_dict_manifest.json")) as f:
        ref = {k: v for k, v in json.load(f).items() if k.startswith("backbone.")}
    assert names == ref                                   # exactly the reference checkpoint layout
    assert lib.fd_model_set_param(h, b"backbone.nope", None, 0) != 0
    bad = np.zeros(3, np.float32)
    assert lib.fd_model_set_param(h, b"backbone.all_modules.0.W", bad.ctypes.data_as(C.c_void_p), 3) != 0
    assert b"expects 64" in lib.fd_last_error()
    lib.fd_model_destroy(h)
    cfg.nf = 12
    assert lib.fd_model_create(C.byref(cfg), C.byref(h)) != 0   # unsupported width -> error code, not a crash


def test_python_api_mirrors_reference_layout():
    import flowdec_amd
    m = flowdec_amd.from_preset("flowdec_75m")
    with open(os.path.join(GOLDEN, "state_dict_manifest.json")) as f:
        ref = json.load(f)
    ours = {k: list(v.shape) for k, v in m.state_dict().items()}
    assert ours == ref                                     # incl. feature_extractor.complex_stft.window, sigma_x, sigma_y
    assert m.sigma_y.dtype == torch.float64 and m.sigma_y.shape == (768, 1) and m.sampling_rate == 48000
    g = load_golden("g12_sigma_y.npz")
    assert np.allclose(m.sigma_y.numpy(), g["75m"], rtol=1e-12)
    assert np.allclose(flowdec_amd.from_preset("flowdec_25s").sigma_y.numpy(), g["25s"], rtol=1e-12)
    assert float(flowdec_amd.from_preset("flowdec_75m_globsigy").sigma_y) == pytest.approx(0.66)
    g1 = load_golden("g1_stft.npz")
    assert np.array_equal(m.feature_extractor.complex_stft.window.numpy(), g1["window"])
    assert sum(p.numel() for p in m.backbone.parameters()) == 23703704
    # a reference checkpoint dict loads with the reference's own call
    sd = {k: torch.zeros(v) for k, v in ref.items()}
    sd["sigma_y"] = sd["sigma_y"].double()
    res = m.load_state_dict(sd)
    assert not res.missing_keys and not res.unexpected_keys


def test_unsupported_configs_and_cpu_refusal():
    import flowdec_amd
    from flowdec_amd.model import BACKBONE_FINAL_NO_ATTN, NCSNpp
    for bad in (dict(attn_resolutions=(768,)), dict(resblock_type="ddpm"), dict(progressive="residual"), dict(nonlinearity="elu")):
        kw = dict(BACKBONE_FINAL_NO_ATTN); kw.update(bad)
        with pytest.raises(NotImplementedError):
            NCSNpp(**kw)
    m = flowdec_amd.from_preset("flowdec_75m", nf=8)
    with pytest.raises(RuntimeError):                       # no CPU compute path: must fail loudly, not fall back
        m.enhance(torch.zeros(1, 1, 24000), N=1)
    with pytest.raises(RuntimeError):
        m(torch.zeros(1, 1, 768, 64, dtype=torch.complex64), torch.zeros(1, 1, 768, 64, dtype=torch.complex64), torch.tensor(0.5))
    from flowdec_amd import op
    with pytest.raises(RuntimeError):
        op.upfirdn2d(torch.zeros(1, 1, 4, 4), torch.ones(4, 4))


def test_shard_ranges():
    from flowdec_amd.dist import shard_range, shard_sizes
    for n, w in ((256, 8), (64, 8), (8, 8), (10, 4), (3, 8), (0, 2)):
        spans = [shard_range(n, r, w) for r in range(w)]
        assert spans[0][0] == 0 and spans[-1][1] == n
        assert all(a[1] == b[0] for a, b in zip(spans, spans[1:]))
        assert max(shard_sizes(n, w)) - min(shard_sizes(n, w)) <= 1


_WORKER = r'''
import os, sys, torch, torch.distributed as dist
sys.path.insert(0, sys.argv[1])
from flowdec_amd.dist import sharded_apply
dist.init_process_group("gloo", rank=int(os.environ["RANK"]), world_size=int(os.environ["WORLD_SIZE"]))
torch.manual_seed(0)
y = torch.randn(5, 1, 100)                       # 5 clips over 2 ranks: uneven shards (3 + 2)
fn = lambda yb: yb * yb.abs().amax(dim=(1, 2), keepdim=True) + 1.0   # per-clip op, like enhance(): no cross-batch term
full = sharded_apply(fn, y)
assert full.shape == y.shape and torch.equal(full, fn(y)), "sharded result differs from the single-process result"
empty = sharded_apply(fn, y[:1])                 # fewer clips than ranks: one rank idles
assert torch.equal(empty, fn(y[:1]))

# sharded_enhance: N ranks == one process, bit for bit, for every way of defining the initial noise.  The model is a stand-in
# with the FlowModel surface sharded_enhance uses (device, feature_extractor._cfg(), enhance(y, N, solver, noise)); the real
# one needs a GPU (tests/test_hip_dist.py).
from flowdec_amd.dist import clip_noise, sharded_enhance
class FE:
    def _cfg(self): return dict(n_fft=30, hop=8, alpha=0.3, beta=0.33)
class Stub:
    device = torch.device("cpu"); feature_extractor = FE(); calls = []
    def enhance(self, yb, N=50, solver="euler", noise=None, **kw):
        assert noise.shape == (yb.shape[0], 1, 16, 64) and noise.dtype == torch.complex64, noise.shape
        self.calls.append(yb.shape[0])
        return yb * N + noise.real.mean(dim=(1, 2, 3)).reshape(-1, 1, 1) + (1.0 if solver == "midpoint" else 0.0)
m = Stub()
y = torch.randn(5, 1, 100)
nz = torch.randn(5, 1, 16, 64, dtype=torch.complex64)
ref = m.enhance(y, N=3, solver="midpoint", noise=nz)
out = sharded_enhance(m, y, N=3, solver="midpoint", noise=nz)
assert torch.equal(out, ref), "noise= mode"
ref = m.enhance(y, N=2, noise=torch.stack([clip_noise(77, i, (1, 16, 64), "cpu") for i in range(5)]))
st = {}
assert torch.equal(sharded_enhance(m, y, N=2, seed=77, stats=st), ref), "seed= mode: clip i draws from stream (seed, i)"
assert st["local_s"] >= 0 and st["gather_s"] > 0
g1 = torch.Generator().manual_seed(5); g2 = torch.Generator().manual_seed(5)
ref = m.enhance(y, N=2, noise=torch.randn((5, 1, 16, 64), dtype=torch.complex64, generator=g1))
assert torch.equal(sharded_enhance(m, y, N=2, generator=g2), ref), "generator= mode: full draw, sliced"
a = sharded_enhance(m, y, N=2); b = sharded_enhance(m, y, N=2)      # nothing given: rank 0's seed is broadcast
ga = [torch.empty_like(a) for _ in range(2)]; dist.all_gather(ga, a)
assert torch.equal(ga[0], ga[1]) and not torch.equal(a, b), "default: all ranks agree on a fresh seed per call"
# generator= with an idle rank (one clip, two ranks): the idle rank draws and discards, so both generators stay identical and the
# NEXT call still equals the single-process sequence of draws
g1 = torch.Generator().manual_seed(9); g2 = torch.Generator().manual_seed(9)
r1 = m.enhance(y[:1], N=2, noise=torch.randn((1, 1, 16, 64), dtype=torch.complex64, generator=g1))
r2 = m.enhance(y, N=2, noise=torch.randn((5, 1, 16, 64), dtype=torch.complex64, generator=g1))
assert torch.equal(sharded_enhance(m, y[:1], N=2, generator=g2), r1)
assert torch.equal(sharded_enhance(m, y, N=2, generator=g2), r2), "generator= after a call with an idle rank"
one = sharded_enhance(m, y[:1], N=2, seed=1)      # one clip, two ranks: rank 1 idles but still gathers
assert one.shape == (1, 1, 100) and torch.equal(one, m.enhance(y[:1], N=2, noise=clip_noise(1, 0, (1, 16, 64), "cpu")[None]))
# a CPU all-reduce as the closing barrier: dist.barrier() probes for an accelerator, which opens the GPU on a GPU machine
dist.all_reduce(torch.zeros(1)); dist.destroy_process_group()
print("rank", os.environ["RANK"], "ok")
'''


def test_batch_sharding_gloo_world2(tmp_path):
    script = tmp_path / "worker.py"
    script.write_text(_WORKER)
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29517", WORLD_SIZE="2")
    procs = [subprocess.Popen([sys.executable, str(script), ROOT], env=dict(env, RANK=str(r)), stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
             for r in range(2)]
    outs = [p.communicate(timeout=120)[0].decode() for p in procs]
    assert all(p.returncode == 0 for p in procs), "\n".join(outs)
    assert all("ok" in o for o in outs)


def test_gather_without_process_group_is_a_clear_error():
    from flowdec_amd.dist import all_gather_shards, sharded_apply, sharded_enhance
    x = torch.zeros(2, 1, 8)
    with pytest.raises(RuntimeError, match="process group"):
        all_gather_shards(x, 2)
    with pytest.raises(RuntimeError, match="process group"):
        sharded_apply(lambda v: v, x, always_gather=True)

    class FE:
        def _cfg(self):
            return dict(n_fft=30, hop=8)

    class Stub:
        device = torch.device("cpu"); feature_extractor = FE()

        def enhance(self, yb, N=50, solver="euler", noise=None, **kw):
            return yb

    with pytest.raises(RuntimeError, match="process group"):
        sharded_enhance(Stub(), x, N=1, seed=0, always_gather=True)
    assert torch.equal(sharded_enhance(Stub(), x, N=1, seed=0), x)      # world 1 without a group: plain call


_WORKER8 = r'''
import os, sys, torch, torch.distributed as dist
sys.path.insert(0, sys.argv[1])
from flowdec_amd.dist import clip_noise, shard_range, sharded_enhance
rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
dist.init_process_group("gloo", rank=rank, world_size=world)
class FE:
    def _cfg(self): return dict(n_fft=30, hop=8)
class Stub:   # the FlowModel surface sharded_enhance uses; records the shard sizes it was called with
    device = torch.device("cpu"); feature_extractor = FE()
    def __init__(self): self.calls = []
    def enhance(self, yb, N=50, solver="euler", noise=None, **kw):
        self.calls.append(yb.shape[0])
        return yb * N + noise.real.mean(dim=(1, 2, 3)).reshape(-1, 1, 1)
# BASELINE cfg 4 (256 clips) and cfg 5 (64 clips) over the 8 ranks of one node, plus an uneven global batch: every rank gets its
# contiguous slice, the gathered result equals the single-process call bit for bit, noise belongs to the GLOBAL clip index
for B, per in ((256, 32), (64, 8), (20, None)):
    torch.manual_seed(B)
    y = torch.randn(B, 1, 40)
    m = Stub()
    out = sharded_enhance(m, y, N=3, solver="midpoint", seed=11)
    lo, hi = shard_range(B, rank, world)
    assert m.calls == [hi - lo] and (per is None or hi - lo == per), (m.calls, lo, hi)
    ref = Stub().enhance(y, N=3, noise=torch.stack([clip_noise(11, i, (1, 16, 64), "cpu") for i in range(B)]))
    assert out.shape == (B, 1, 40) and torch.equal(out, ref), B
# a CPU all-reduce as the closing barrier: dist.barrier() probes for an accelerator, which opens the GPU on a GPU machine
dist.all_reduce(torch.zeros(1)); dist.destroy_process_group()
print("rank", rank, "ok")
'''


def test_batch_sharding_gloo_world8_cfg4_cfg5(tmp_path):
    """The 8-rank splits of BASELINE cfg 4 (256 x 2 s -> 32 clips per GPU) and cfg 5 (64 x 4 s -> 8 per GPU) through
    `sharded_enhance` on the CPU (gloo, stand-in model): shard sizes, gather order, noise by global clip index."""
    script = tmp_path / "worker8.py"
    script.write_text(_WORKER8)
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29531", WORLD_SIZE="8", OMP_NUM_THREADS="1")
    procs = [subprocess.Popen([sys.executable, str(script), ROOT], env=dict(env, RANK=str(r)), stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
             for r in range(8)]
    outs = [p.communicate(timeout=240)[0].decode() for p in procs]
    assert all(p.returncode == 0 for p in procs), "\n".join(outs)
    assert all("ok" in o for o in outs)


def test_bench_self_launch_gloo_world2():
    """`python bench.py --gpus 2` WITHOUT a launcher runs torch.distributed.run with two ranks as a child process, shards the
    global batch by clip, all-gathers the results inside the timed region and prints ONE line with n_gpus = the real world size
    (here: gloo + a stub step, the model needs a GPU; the code path -- relaunch, sharded_apply, timing reduction -- is the
    one the multi-GPU bench takes)."""
    import json
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--backend", "gloo", "--stub-step", "--steps", "2",
                        "--warmup", "1", "--seconds", "0.01", "--batch", "3"], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    res = json.loads(lines[0])
    assert res["n_gpus"] == 2 and res["config"]["global_batch"] == 6 and res["scaling"] == "weak" and len(res["per_rank_ms_per_step"]) == 2
    assert res["config"]["parallelism"] == "batch-shard x2" and res["allgather_ms_per_step"] > 0
    # strong scaling form: the global batch is fixed and split
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--backend", "gloo", "--stub-step", "--steps", "1",
                        "--warmup", "0", "--seconds", "0.01", "--global-batch", "5"], env=env, capture_output=True, text=True, timeout=300)
    res = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][0])
    assert res["n_gpus"] == 2 and res["config"]["global_batch"] == 5 and res["scaling"] == "strong"
    # BASELINE config 4's shape arithmetic: 256 clips over the ranks (2 here, 8 on the node), strong scaling
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--backend", "gloo", "--stub-step", "--steps", "1",
                        "--warmup", "0", "--seconds", "0.01", "--global-batch", "256", "--N", "3", "--solver", "midpoint"], env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    res = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][0])
    assert res["n_gpus"] == 2 and res["config"]["global_batch"] == 256 and res["config"]["clips_per_rank"] == [128, 128]
    assert res["scaling"] == "strong" and res["config"]["nfe"] == 6 and abs(res["value"] * res["ms_per_step"] * 1e-3 - 256 * 0.01) < 1e-6


def test_bench_config_flag_cfg4_shard_line():
    """`bench.py --gpus N --config cfg4` is BASELINE config 4 in one command: FlowDec-75m, 32 x 2 s clips PER RANK (8 ranks = the 256-clip
    batch), midpoint N = 6 = 12 evaluations (the reference counts solver steps, flowdec/model.py:487; `cfg4_nfe6` is the N = 3 reading), bf16,
    weak scaling; explicit flags still win over the named configuration, abbreviated flags are refused (gloo + stub step here)."""
    import json
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--config", "cfg4", "--backend", "gloo", "--stub-step",
                        "--steps", "1", "--warmup", "0", "--seconds", "0.01"], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    res = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][0])
    assert res["n_gpus"] == 2 and res["config"]["clips_per_rank"] == [32, 32] and res["config"]["global_batch"] == 64
    assert res["config"]["nfe"] == 12 and res["scaling"] == "weak" and res["dtype"] == "bf16"
    sys.path.insert(0, ROOT)
    import bench
    assert bench.CONFIGS["cfg4"] == dict(preset="flowdec_75m", batch=32, seconds=2.0, N=6, solver="midpoint", precision="bf16")
    assert bench.CONFIGS["cfg4_nfe6"]["N"] == 3 and bench.CONFIGS["cfg3"]["N"] == 6 and bench.CONFIGS["cfg3_nfe6"]["N"] == 3
    assert bench.CONFIGS["cfg5_dopri5"]["solver"] == "dopri5" and bench.CONFIGS["cfg3_n6"] == bench.CONFIGS["cfg3"]
    # an abbreviated flag ("--prec") would slip past the override test of --config: argparse must refuse it
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--config", "cfg4", "--prec", "fp32", "--stub-step"], env=env,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "unrecognized arguments" in r.stderr
    assert bench.CONFIGS["cfg5"]["precision"] == "fp32" and bench.CONFIGS["cfg5"]["seconds"] == 4.0 and bench.CONFIGS["cfg3"]["preset"] == "flowdec_25s"


def test_bench_dump_outputs(tmp_path, monkeypatch):
    """`bench.py --dump-outputs DIR` writes what the LAST timed step returned as DIR/waveform.npy (float32 [B, 1, L]): the stub step
    returns 2 y + k at step k, so the warm-up and the earlier timed steps are told apart.  The same bytes for the same arguments,
    the same array under two ranks (gloo + a stub step here); --steps 0 is refused; beyond the budget the files on disk, headers
    included, stay within DUMP_MAX_BYTES and hold a fixed, seeded sample."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT")}
    common = ["--backend", "gloo", "--stub-step", "--steps", "3", "--warmup", "1", "--seconds", "0.01", "--global-batch", "5"]
    for d, gpus in (("a", "1"), ("b", "1"), ("c", "2")):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", gpus, *common, "--dump-outputs", str(tmp_path / d)],
                           env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        assert json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][0])["steps"] == 3
    a = np.load(tmp_path / "a" / "waveform.npy")
    y = 0.1 * torch.randn(5, 1, 480, generator=torch.Generator().manual_seed(0))      # the stub's seeded global batch
    assert a.dtype == np.float32 and a.shape == (5, 1, 480) and np.array_equal(a, (y * 2.0 + 2).numpy())   # step k = steps - 1 = 2
    assert (tmp_path / "a" / "waveform.npy").read_bytes() == (tmp_path / "b" / "waveform.npy").read_bytes()
    assert np.array_equal(np.load(tmp_path / "c" / "waveform.npy"), a)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--stub-step", "--steps", "0"], env=env, capture_output=True, text=True,
                       timeout=120)
    assert r.returncode != 0 and "--steps" in r.stderr
    sys.path.insert(0, ROOT)
    import bench
    on_disk = lambda d: sum(os.path.getsize(f) for f in d.iterdir())
    # BASELINE cfg 4 on 8 GPUs: 256 x 2 s clips = 98.3 MB of float32 -> a sample within the real budget
    bench.dump_outputs(str(tmp_path / "big"), {"waveform": np.zeros((256, 1, 96000), np.float32)})
    assert on_disk(tmp_path / "big") <= bench.DUMP_MAX_BYTES <= 64 * 10 ** 6
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", bench.DUMP_HEADER_BYTES + 4000)
    x = np.arange(3 * 1000, dtype=np.float32).reshape(3, 1, 1000)
    bench.dump_outputs(str(tmp_path / "s1"), {"waveform": x})
    bench.dump_outputs(str(tmp_path / "s2"), {"waveform": x})
    s = np.load(tmp_path / "s1" / "waveform.npy")
    assert on_disk(tmp_path / "s1") <= bench.DUMP_MAX_BYTES and s.dtype == np.float32 and s.size == 1000
    assert np.all(np.diff(s) > 0) and np.isin(s, x).all() and np.array_equal(s, np.load(tmp_path / "s2" / "waveform.npy"))


def test_bench_full_flag_is_off_by_default():
    """`--full` (everything the headline figure does not need: calibration / power, e2e, rooflines, CPU baseline) is an option of its
    own, off by default; none of what it adds applies to the stub step, so the line has the same keys with and without it."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT")}
    keys = []
    for flags in ([], ["--full"]):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--stub-step", "--steps", "1", "--warmup", "0", "--seconds", "0.01",
                            *flags], env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        keys.append(sorted(json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][0])))
    assert keys[0] == keys[1] and not {"cpu_baseline", "roofline", "e2e", "box_calibration", "power"} & set(keys[0])


def test_bench_refuses_missing_gpus():
    """Never a silent N = 1 line: asking for more GPUs than the box has must fail loudly (this container has none)."""
    import torch
    if torch.cuda.device_count() >= 2:
        pytest.skip("box has the GPUs")
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0"], env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "refusing" in (r.stdout + r.stderr) and "{" not in r.stdout


def test_parity_metrics_match_reference():
    """SI-SDR / SI-SIR / SI-SAR equal the reference's eval/metrics.py SISXR on the golden signals; logspec_mse properties."""
    from conftest import load_golden
    from flowdec_amd import metrics
    g = load_golden("g14_metrics.npz")
    for i in range(3):
        got = metrics.si_sxr(g[f"xhat{i}"], g[f"x{i}"], g[f"y{i}"])
        np.testing.assert_allclose(got, g[f"sisxr{i}"], rtol=0, atol=1e-4)
    x = g["x0"]
    assert metrics.si_sdr(0.5 * x, x) > 100 and abs(metrics.si_sdr(x + 0.1 * g["x1"], x) - 20.0) < 0.5
    assert metrics.logspec_mse(x, x) == 0.0 and metrics.logspec_mse(2 * x, x) == pytest.approx((20 * np.log10(2)) ** 2, rel=1e-3)


def test_c_abi_from_plain_c(tmp_path):
    """include/flowdec_hip.h is valid C99 and the library is usable from a plain C host (dlopen + dlsym), the way a
    cgo / JNI / C++ integration of the reference would bind it."""
    import subprocess
    from flowdec_amd import _lib
    _lib.load()
    here = os.path.dirname(os.path.abspath(__file__))
    exe = str(tmp_path / "abi_check")
    inc = os.path.join(here, "..", "include")
    hdr_only = tmp_path / "hdr.c"
    hdr_only.write_text('#include "flowdec_hip.h"\nint main(void) { fd_model_config c; fd_score_config s; (void)c; (void)s; return 0; }\n')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-fsyntax-only", "-I", inc, str(hdr_only)], check=True)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", inc, os.path.join(here, "c", "abi_check.c"), "-o", exe, "-ldl"], check=True)
    r = subprocess.run([exe, _lib.LIB_PATH], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    assert "c abi ok" in r.stdout


def test_wino4_kernel_owns_m0():
    """conv_wino4.hip writes M0 from inline asm without saving it and counts its own vector-memory waits: the ISA properties that
    makes safe are checked by the BUILD itself (flowdec_amd/build.py check_wino4_isa: no foreign M0 use, no scratch, one set of MFMA
    sites per instantiation) -- here the same check as a test."""
    import shutil
    from flowdec_amd import build as B
    if not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")):
        pytest.skip("hipcc not available")
    assert B.check_wino4_isa()


def test_every_committed_profile_json_parses():
    """profiles/*.json are the evidence the bench lines and DESIGN / MEASUREMENTS cite: each must be one valid JSON document."""
    import glob
    import json
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", "*.json")))
    assert files
    for f in files:
        with open(f) as fh:
            json.load(fh)
