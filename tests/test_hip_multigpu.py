"""The corpus path over several ranks on the hardware that exists (one MI355X per test box): ranks SHARE the GPU.

  * `sharded_enhance_batch` (7 clips in two T_pad buckets, batches of 2) and `sharded_enhance_long` ([2, 1, L], 3 rows per channel) over 2
    and 3 gloo ranks == the one-process calls, as int32 views;
  * `enhance_cli --gpus N --share-gpu` == the one-process run: the same set of output files with the same bytes, the same rtfs.csv paths
    in the same order, the same triples list and counts, no part file left; more ranks than batches; more GPUs asked for than there are;
    a worker that fails on one file.
Everything runs the nf-8 model of `synthetic_ckpt()` on 64- and 128-frame images: process start-up dominates.  The launcher logic that
needs no GPU (plan, merge, manifest, argument checks): tests/test_dist_corpus_cpu.py.
"""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

pytestmark = pytest.mark.gpu

_COMMON = r'''
import os, sys, torch, torch.distributed as dist
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
from test_cli import synthetic_ckpt
from flowdec_amd import enhance_cli
from flowdec_amd.dist import sharded_enhance_batch, sharded_enhance_long
from flowdec_amd.noise import clip_seed, seeds_to_tensor
rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
torch.cuda.set_device(0)
dist.init_process_group("gloo", rank=rank, world_size=world)

def build(kind, precision="bf16"):
    ckpt = synthetic_ckpt()
    for sd in (ckpt["state_dict"], ckpt["_pl_ema_state_dict"]):      # keeps a sampler on random weights in range
        sd["backbone.output_layer.weight"] = sd["backbone.output_layer.weight"] * 0.02
    return enhance_cli.model_from_checkpoint(ckpt, precision=precision, model=kind).cuda()

def bits(t): return t.detach().cpu().contiguous().view(torch.int32)

def same(a, b): return a.shape == b.shape and a.device == b.device and torch.equal(bits(a), bits(b))

def finish():
    # a CPU all-reduce as the closing barrier
    dist.all_reduce(torch.zeros(1)); dist.destroy_process_group()
    print("rank", rank, "ok")
'''

_BATCH = _COMMON + r'''
# two buckets: < 24576 samples -> 64 frames (clips 0, 2, 5), 24576 .. 49151 -> 128 (clips 1, 3, 4, 6); batches of 2: [0 2] [5] [1 3] [4 6]
LENS = [12000, 30000, 24575, 24576, 49151, 20000, 41234]
g = torch.Generator().manual_seed(5)
clips = [0.1 * torch.randn(n, generator=g) for n in LENS]
clips[1] = clips[1].reshape(1, -1); clips[3] = clips[3].reshape(1, 1, -1)       # [L], [1, L] and [1, 1, L]
clips[2] = clips[2].cuda(); clips[4] = clips[4].cuda()                          # host and device inputs
seeds = [clip_seed(9, i) for i in range(7)]
CASES = [("flow", "bf16", dict(N=2, solver="midpoint")), ("flow", "fp32", dict(N=2, solver="midpoint")), ("score", "bf16", dict(N=2)),
         ("regression", "bf16", dict()), ("flow", "bf16", dict(N=2, solver="dopri5", step_control="clip", atol=1e-2, rtol=1e-2))]
for kind, precision, kw in CASES:
    m = build(kind, precision)
    ref = [m.enhance(c, **kw) if kind == "regression" else m.enhance(c, seed=[s], **kw) for c, s in zip(clips, seeds)]
    assert all(torch.isfinite(r).all() and r.abs().max() > 0 for r in ref), (kind, precision)
    st = {}
    out = sharded_enhance_batch(m, clips, batch_clips=2, seed=9, stats=st, **kw)
    assert st["plan"] == [[0, 2], [5], [1, 3], [4, 6]] and len(out) == 7
    for i in range(7):
        assert same(out[i], ref[i]) and out[i].shape == clips[i].shape and out[i].device == clips[i].device, (kind, precision, kw, i)
    if kind == "flow" and precision == "bf16" and kw["solver"] == "midpoint":
        out = sharded_enhance_batch(m, clips, batch_clips=2, seeds=seeds_to_tensor(seeds, 7, "cpu"), **kw)      # seeds=: one per clip, here as an int64 tensor
        assert all(same(o, r) for o, r in zip(out, ref))
        solo = sharded_enhance_batch(m, clips[6:], seeds=seeds[6:], **kw)                          # one clip: the other ranks idle
        assert len(solo) == 1 and same(solo[0], ref[6])
        a = torch.cat([o.reshape(-1).cpu() for o in sharded_enhance_batch(m, clips, batch_clips=2, **kw)])   # seed=None: rank 0's, broadcast
        ga = [torch.empty_like(a) for _ in range(world)]; dist.all_gather(ga, a)
        assert all(torch.equal(bits(x), bits(ga[0])) for x in ga)
    del m
finish()
'''

_LONG = _COMMON + r'''
m = build("flow")
g = torch.Generator().manual_seed(6)
y = 0.1 * torch.randn(2, 1, 48000, generator=g)
y[1] *= 0.5                                                                          # two channels, two normalisations
geo = dict(row_frames=64, halo_frames=16)
assert m.enhance_long_jobs(y, **geo) == 6                                            # 3 rows per channel
kw = dict(N=2, solver="midpoint", **geo)
ref = m.enhance_long(y, seed=5, **kw)
assert torch.isfinite(ref).all() and ref.abs().max() > 0
assert same(sharded_enhance_long(m, y, seed=5, **kw), ref), "sharded rows != enhance_long"
assert same(sharded_enhance_long(m, y, seed=5, rows_per_call=1, **kw), ref), "rows_per_call=1"
assert same(sharded_enhance_long(m, y.cuda(), seed=5, **kw), ref.cuda()), "device input"
# the two halves on their own: any split of the jobs stitches to the same bits
rows = torch.cat([m.enhance_long_rows(y, jobs=(lo, hi), seed=5, **kw) for lo, hi in ((0, 1), (1, 5), (5, 6))])
assert same(m.enhance_long_stitch(y, rows, **geo), ref)
a = sharded_enhance_long(m, y, **kw).reshape(-1)                                      # seed=None: rank 0 draws, every rank agrees
ga = [torch.empty_like(a) for _ in range(world)]; dist.all_gather(ga, a)
assert all(torch.equal(bits(x), bits(ga[0])) for x in ga) and not torch.equal(a, ref.reshape(-1))
finish()
'''


def _port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _clean_env(**kw):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.update(kw)
    return env


def _run_ranks(tmp_path, text, world):
    script = tmp_path / "ranks.py"
    script.write_text(text)
    env = _clean_env(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_port()), WORLD_SIZE=str(world), HSA_ENABLE_IPC_MODE_LEGACY="0")
    procs = [subprocess.Popen([sys.executable, str(script), ROOT], env=dict(env, RANK=str(r)), stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
             for r in range(world)]
    outs = [p.communicate(timeout=600)[0].decode() for p in procs]
    assert all(p.returncode == 0 for p in procs), "\n".join(o[-3000:] for o in outs)
    assert all("ok" in o for o in outs)


@pytest.mark.parametrize("world", [2, 3])
def test_sharded_enhance_batch_bit_identical(tmp_path, world):
    """FlowModel (midpoint: bf16 and fp32; dopri5 with per-clip step control), ScoreModel and RegressionModel: the sharded list equals
    `[model.enhance(c, seed=[s_i])]` as int32 views on every rank, shapes and devices kept."""
    _run_ranks(tmp_path, _BATCH, world)


@pytest.mark.parametrize("world", [2, 3])
def test_sharded_enhance_long_bit_identical(tmp_path, world):
    """6 (channel, row) jobs over 2 and 3 ranks == enhance_long, also with rows_per_call=1 and from a device input."""
    _run_ranks(tmp_path, _LONG, world)


# ------------------------------------------------------------------------------------------------
# enhance_cli --gpus N --share-gpu
# ------------------------------------------------------------------------------------------------
# the nine files of test_cli_batches_files_bit_identical_to_one_file_per_call (tests/test_hip_ragged.py)
NINE = [("a", 30000, 48000, 1), ("b", 41234, 48000, 1), ("c", 24576, 48000, 1), ("d", 49151, 48000, 1), ("e", 48000, 48000, 1),
        ("f", 20000, 48000, 1), ("g", 23000, 48000, 1), ("h", 12000, 16000, 1), ("long", 31 * 8000, 8000, 1)]
ROWS = ("zrows", 60000, 48000, 1)            # 1.25 s: the long-form path under --chunk-seconds 0.6 --max-seconds 1
STEREO = ("stereo", 20000, 48000, 2)


def _write_corpus(ind, spec, seed=2):
    from flowdec_amd import enhance_cli
    ind.mkdir()
    rng = np.random.default_rng(seed)
    for name, n, sr, ch in spec:
        enhance_cli.save_wav(str(ind / f"{name}.wav"), torch.from_numpy((0.1 * rng.standard_normal((ch, n))).astype(np.float32)), sr)


def _ckpt(tmp_path, target=None, **hp):
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from test_cli import synthetic_ckpt
    ckpt = synthetic_ckpt()
    if target:
        ckpt["hyper_parameters"]["model"]["_target_"] = target
        for sd in (ckpt["state_dict"], ckpt["_pl_ema_state_dict"]):     # keeps a sampler on random weights in range
            sd["backbone.output_layer.weight"] = sd["backbone.output_layer.weight"] * 0.02
    ckpt["hyper_parameters"]["model"].update(hp)
    torch.save(ckpt, tmp_path / "m.ckpt")
    return str(tmp_path / "m.ckpt")


def _launch(argv):
    """`python -m flowdec_amd.enhance_cli argv` as a child: the launcher of a --gpus N run must be a process that never opens the GPU."""
    env = _clean_env(PYTHONPATH=ROOT + (os.pathsep + os.environ["PYTHONPATH"] if os.environ.get("PYTHONPATH") else ""))
    return subprocess.run([sys.executable, "-m", "flowdec_amd.enhance_cli"] + argv, env=env, capture_output=True, text=True, timeout=600)


def _wavs(d):
    return {f: (d / f).read_bytes() for f in sorted(os.listdir(d)) if f.endswith(".wav")}


def _rtf_paths(d):
    return [ln.split(",")[0].split("/")[-1] for ln in (d / "rtfs.csv").read_text().strip().splitlines()[1:]]


def _assert_same_run(one_dir, many_dir, res_one, child, expect_files):
    assert child.returncode == res_one.exit_code, (child.stdout + child.stderr)[-3000:]
    assert sorted(os.listdir(one_dir)) == sorted(os.listdir(many_dir)), (os.listdir(one_dir), os.listdir(many_dir))      # no part file, no manifest
    one, many = _wavs(one_dir), _wavs(many_dir)
    assert sorted(one) == sorted(many) == sorted(f"{n}.wav" for n in expect_files)
    for f in one:
        assert one[f] == many[f], f"{f}: the --gpus N output differs from the one-process output"
    assert _rtf_paths(one_dir) == _rtf_paths(many_dir) and len(_rtf_paths(one_dir)) == res_one.n_done == len(expect_files)
    total = [ln for ln in child.stdout.splitlines() if ln.startswith("total: ")]
    assert len(total) == 1 and total[0].startswith(f"total: {res_one.audio_seconds:.2f} s of audio in "), child.stdout[-2000:]
    assert sum(ln.startswith("[rank ") and "Done loading model." in ln for ln in child.stdout.splitlines()) > 1


def test_cli_corpus_three_workers_equal_one_process(tmp_path):
    """The corpus of nine files (two buckets, one resampled, one of 31 s) plus a 1.25 s file, with `--chunk-seconds 0.6 --max-seconds 1
    --rng native --seed 3 --rtf` (every file over 0.51 s runs in rows), and the nine files again with `--rng torch --seed 11` (ragged
    batches): `--gpus 3 --share-gpu` in a child against the one-process run."""
    from flowdec_amd import enhance_cli
    ckpt = _ckpt(tmp_path)
    _write_corpus(tmp_path / "in", NINE + [ROWS])
    common = ["--ckpt", ckpt, "--files", str(tmp_path / "in"), "--N", "2", "--solver", "midpoint", "--rtf", "--batch-files", "4"]
    native = common + ["--rng", "native", "--seed", "3", "--chunk-seconds", "0.6", "--max-seconds", "1"]
    r1 = enhance_cli.run(native + ["--outdir", str(tmp_path / "n1"), "--gpus", "1"])
    assert r1.n_done == 10 and r1.exit_code == 0
    child = _launch(native + ["--outdir", str(tmp_path / "n3"), "--gpus", "3", "--share-gpu"])
    _assert_same_run(tmp_path / "n1", tmp_path / "n3", r1, child, [s[0] for s in NINE + [ROWS]])
    assert "3 workers: " in child.stdout and "Long file:" in child.stdout
    os.remove(tmp_path / "in" / "zrows.wav")
    gens = common + ["--rng", "torch", "--seed", "11"]
    r1 = enhance_cli.run(gens + ["--outdir", str(tmp_path / "t1"), "--gpus", "1"])
    assert r1.n_done == 8 and r1.n_too_long == 1
    child = _launch(gens + ["--outdir", str(tmp_path / "t3"), "--gpus", "3", "--share-gpu"])
    _assert_same_run(tmp_path / "t1", tmp_path / "t3", r1, child, [s[0] for s in NINE[:-1]])
    assert child.stdout.count("Skipping file due to length:") == 1


def test_cli_scoredec_pair_list_two_workers(tmp_path):
    """A ScoreDec checkpoint (N = 2) and a pair list: `--gpus 2 --share-gpu` writes the one-process files, rtfs.csv and triples_list.txt."""
    from flowdec_amd import enhance_cli
    ckpt = _ckpt(tmp_path, "flowdec.model.ScoreModel", sde=dict(_target_="flowdec.sdes.OUVESDE", theta=1.5, sigma_min=0.05, sigma_max=0.5, N=30),
                 t_eps=0.03)
    spec = [("a", 12000, 48000, 1), ("b", 20000, 48000, 1), ("c", 30000, 48000, 1), ("d", 12000, 48000, 1), ("e", 30000, 48000, 1)]
    _write_corpus(tmp_path / "in", spec)
    pairs = tmp_path / "pairs.txt"
    pairs.write_text("".join(f"/clean/{n}.wav ---> {tmp_path / 'in' / (n + '.wav')}\n" for n, *_ in spec))
    common = ["--ckpt", ckpt, "--files", str(pairs), "--N", "2", "--rtf", "--rng", "native", "--seed", "3", "--batch-files", "2"]
    r1 = enhance_cli.run(common + ["--outdir", str(tmp_path / "o1")])
    assert r1.n_done == 5
    child = _launch(common + ["--outdir", str(tmp_path / "o2"), "--gpus", "2", "--share-gpu"])
    assert "model=ScoreModel" in child.stdout
    _assert_same_run(tmp_path / "o1", tmp_path / "o2", r1, child, [s[0] for s in spec])
    t1, t2 = (tmp_path / "o1" / "triples_list.txt").read_text(), (tmp_path / "o2" / "triples_list.txt").read_text()
    assert t1.replace(str(tmp_path / "o1"), "OUT") == t2.replace(str(tmp_path / "o2"), "OUT") and len(t1.splitlines()) == 5


def test_cli_more_workers_than_batches(tmp_path):
    """Two files (one batch) on four workers: three of them idle, exit 0, and the bytes are the one-process bytes."""
    from flowdec_amd import enhance_cli
    ckpt = _ckpt(tmp_path)
    _write_corpus(tmp_path / "in", [("f", 20000, 48000, 1), ("g", 23000, 48000, 1)])
    common = ["--ckpt", ckpt, "--files", str(tmp_path / "in"), "--N", "2", "--solver", "midpoint", "--rtf", "--rng", "native", "--seed", "3"]
    r1 = enhance_cli.run(common + ["--outdir", str(tmp_path / "o1")])
    child = _launch(common + ["--outdir", str(tmp_path / "o4"), "--gpus", "4", "--share-gpu"])
    _assert_same_run(tmp_path / "o1", tmp_path / "o4", r1, child, ["f", "g"])
    assert child.stdout.count(": 0 of 1 batches") == 3 and child.stdout.count(": 1 of 1 batches") == 1


def test_cli_refuses_more_gpus_than_visible(tmp_path):
    K = torch.cuda.device_count()
    if K >= 8:
        pytest.skip("a full node: there is no --gpus above its device count to ask for here")
    ckpt = _ckpt(tmp_path)
    _write_corpus(tmp_path / "in", [("f", 20000, 48000, 1)])
    child = _launch(["--ckpt", ckpt, "--files", str(tmp_path / "in"), "--N", "2", "--outdir", str(tmp_path / "o"), "--gpus", str(K + 1)])
    assert child.returncode != 0 and f"--gpus {K + 1}" in child.stderr and f"the {K} visible" in child.stderr, (child.stdout + child.stderr)[-2000:]
    assert "[rank" not in child.stdout and "Loading model" not in child.stdout
    assert not (tmp_path / "o").exists() or os.listdir(tmp_path / "o") == []


def test_cli_worker_failure_leaves_the_rest_finished(tmp_path):
    """One file of four has a truncated header: its worker ends with the exception a one-process run raises, the launcher exits non-zero
    and names the rank, the other three outputs are the one-process bytes, and a rerun without the bad file finds nothing left to do."""
    from flowdec_amd import enhance_cli
    ckpt = _ckpt(tmp_path)
    _write_corpus(tmp_path / "in", [("a", 30000, 48000, 1), ("f", 20000, 48000, 1), ("g", 23000, 48000, 1)])
    (tmp_path / "in" / "bad.wav").write_bytes((tmp_path / "in" / "a.wav").read_bytes()[:20])
    common = ["--ckpt", ckpt, "--files", str(tmp_path / "in"), "--N", "2", "--solver", "midpoint", "--rtf", "--rng", "native", "--seed", "3"]
    with pytest.raises(Exception):            # unreadable files run last, one per call: the three good files are written before it
        enhance_cli.run(common + ["--outdir", str(tmp_path / "o1")])
    assert sorted(_wavs(tmp_path / "o1")) == ["a.wav", "f.wav", "g.wav"]
    child = _launch(common + ["--outdir", str(tmp_path / "o2"), "--gpus", "2", "--share-gpu"])
    assert child.returncode not in (0, 3), child.stdout[-2000:]
    failed = [r for r in (0, 1) if f"rank {r} ended with status 1" in child.stderr]
    assert len(failed) == 1 and "1 of 2 workers failed" in child.stderr and "struct.error" in child.stderr, child.stderr[-3000:]
    assert _wavs(tmp_path / "o1") == _wavs(tmp_path / "o2")
    assert any(".rank" in f for f in os.listdir(tmp_path / "o2"))                    # the parts stay for diagnosis
    os.remove(tmp_path / "in" / "bad.wav")
    again = _launch(common + ["--outdir", str(tmp_path / "o2"), "--gpus", "2", "--share-gpu"])
    assert again.returncode == 0 and "2 workers: 0 files in" in again.stdout, (again.stdout + again.stderr)[-3000:]
    assert sorted(os.listdir(tmp_path / "o2")) == ["a.wav", "f.wav", "g.wav", "rtfs.csv"]
    assert _wavs(tmp_path / "o1") == _wavs(tmp_path / "o2")


def test_cli_two_channel_file_fails_its_worker_like_one_process(tmp_path):
    """A two-channel file ends a one-process run with a RuntimeError (`enhance` takes one channel) after the files planned before it; under
    `--gpus 2` it ends its worker the same way, and the mono file beside it is written by both."""
    from flowdec_amd import enhance_cli
    ckpt = _ckpt(tmp_path)
    _write_corpus(tmp_path / "in2", [STEREO, ("f", 20000, 48000, 1)])
    two = ["--ckpt", ckpt, "--files", str(tmp_path / "in2"), "--N", "2", "--solver", "midpoint", "--rng", "native", "--seed", "3"]
    with pytest.raises(RuntimeError, match="waveforms"):
        enhance_cli.run(two + ["--outdir", str(tmp_path / "s1")])
    child = _launch(two + ["--outdir", str(tmp_path / "s2"), "--gpus", "2", "--share-gpu"])
    assert child.returncode == 1 and "1 of 2 workers failed" in child.stderr and "waveforms" in child.stderr, child.stderr[-3000:]
    assert _wavs(tmp_path / "s1") == _wavs(tmp_path / "s2") and list(_wavs(tmp_path / "s2")) == ["f.wav"]
