"""The corpus path over several ranks, without a GPU: `dist.balance`, `sharded_enhance_batch` over gloo with a stand-in model whose
`enhance` / `enhance_batch` are pure functions of (clip, seed), and the launcher side of `enhance_cli --gpus N` (argument checks, the
manifest, the merge of the workers' part files).  The real model on the GPU: tests/test_hip_multigpu.py."""
import itertools
import json
import os
import socket
import subprocess
import sys

import pytest
import torch

from conftest import ROOT


# ------------------------------------------------------------------------------------------------
# balance
# ------------------------------------------------------------------------------------------------
def test_balance_exhaustive():
    """Every cost vector in {1..4}^n, n <= 6, over 1..4 ranks: a partition, per-rank ascending order, the list-scheduling bound
    max load <= sum / world + max cost, the same plan when asked again, and the identity for one rank."""
    from flowdec_amd.dist import balance
    for world in range(1, 5):
        assert balance([], world) == [[] for _ in range(world)]
        for n in range(1, 7):
            for costs in itertools.product(range(1, 5), repeat=n):
                plan = balance(costs, world)
                assert len(plan) == world and sorted(i for p in plan for i in p) == list(range(n)), (costs, world, plan)
                assert all(p == sorted(p) for p in plan)
                assert max(sum(costs[i] for i in p) for p in plan) <= sum(costs) / world + max(costs), (costs, world, plan)
                assert balance(list(costs), world) == plan
                if world == 1:
                    assert plan == [list(range(n))]


def test_balance_rule_and_ties():
    from flowdec_amd.dist import balance
    # longest first, each to the least-loaded rank: 5 -> r0, 4 -> r1, 3 -> r1 (load 4 < 5), 1 -> r0 (5 < 7), 1 -> r0 (6 < 7)
    assert balance([3, 1, 4, 1, 5], 2) == [[1, 3, 4], [0, 2]]
    # equal costs go in item order, equal loads to the lower rank; more ranks than items leaves ranks empty; zero costs are items too
    assert balance([2, 2, 2, 2], 2) == [[0, 2], [1, 3]]
    assert balance([7], 3) == [[0], [], []]
    assert balance([0, 0, 3], 2) == [[2], [0, 1]]
    with pytest.raises(ValueError):
        balance([1], 0)


# ------------------------------------------------------------------------------------------------
# sharded_enhance_batch over gloo
# ------------------------------------------------------------------------------------------------
_WORKER = r'''
import json, os, sys, torch, torch.distributed as dist
sys.path.insert(0, sys.argv[1])
from flowdec_amd.dist import balance, plan_clip_batches, sharded_enhance_batch
from flowdec_amd.noise import clip_seed
rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
dist.init_process_group("gloo", rank=rank, world_size=world)

class FE:
    def _cfg(self): return dict(n_fft=1534, hop=384, alpha=0.3, beta=0.33)

def one(c, s, N):      # a pure function of (clip, seed): keeps the sign of a zero, differs from clip to clip and from seed to seed
    return c * float(N) * (1.0 + (int(s) % 1009) / 1009.0)

class Stub:            # the surface sharded_enhance_batch uses: device, feature_extractor._cfg(), enhance_batch(clips, seeds=, ...)
    device = torch.device("cpu"); feature_extractor = FE()
    def __init__(self): self.calls = []
    def enhance(self, c, N=50, seed=None, **kw):
        return one(c, seed[0], N)
    def enhance_batch(self, clips, N=50, seeds=None, **kw):
        assert "noise" not in kw and "generator" not in kw and len(seeds) == len(clips)
        self.calls.append([int(c.numel()) for c in clips])
        return [one(c, s, N) for c, s in zip(clips, seeds)]

def bits(t): return t.contiguous().view(torch.int32)

# 7 clips in 3 buckets (T_pad 64: < 24576 samples, 128: < 49152, 192), shapes [L], [1, L] and [1, 1, L], a negative zero in each
LENS = [1000, 30000, 50000, 2000, 31000, 24575, 60000]
g = torch.Generator().manual_seed(3)
clips = [torch.randn(n, generator=g) for n in LENS]
for c in clips: c[7] = -0.0
clips[1] = clips[1].reshape(1, -1); clips[2] = clips[2].reshape(1, 1, -1)
m, st = Stub(), {}
out = sharded_enhance_batch(m, clips, batch_clips=2, seed=21, N=3, stats=st)
ref = [m.enhance(c, N=3, seed=[clip_seed(21, i)]) for i, c in enumerate(clips)]
assert len(out) == 7
for i, (o, r) in enumerate(zip(out, ref)):
    assert o.shape == clips[i].shape and o.dtype == torch.float32 and torch.equal(bits(o), bits(r)), f"clip {i}"
    assert bits(o).reshape(-1)[7].item() == -2 ** 31, "the sign of a zero"
plan = [[0, 3], [5], [1, 4], [2, 6]]
assert st["plan"] == plan and [idx for _, idx in plan_clip_batches(LENS, 384, 2)] == plan
assert st["mine"] == balance([128, 64, 256, 384], world)[rank]
assert m.calls == [[LENS[i] for i in plan[b]] for b in st["mine"]], (m.calls, st)
with open(os.path.join(sys.argv[2], f"ran{world}_{rank}.json"), "w") as f:
    json.dump(m.calls, f)
# seeds= : one per clip, whatever the index
sd = [5, 2 ** 62 + 1, 7, 7, 0, 11, 13]
out = sharded_enhance_batch(m, clips, batch_clips=2, seeds=sd, N=2)
assert all(torch.equal(bits(o), bits(m.enhance(c, N=2, seed=[s]))) for o, c, s in zip(out, clips, sd))
# one clip: every rank but one idles and still takes part (seed broadcast and gather)
m1 = Stub()
solo = sharded_enhance_batch(m1, clips[4:5], seed=None, N=2)
assert len(solo) == 1 and solo[0].shape == clips[4].shape and m1.calls == ([[31000]] if rank == 0 else [])
# nothing given: rank 0 draws a seed, every rank gets the same result; a new seed per call
a = torch.cat([o.reshape(-1) for o in sharded_enhance_batch(m, clips, batch_clips=2, N=2)])
b = torch.cat([o.reshape(-1) for o in sharded_enhance_batch(m, clips, batch_clips=2, N=2)])
ga = [torch.empty_like(a) for _ in range(world)]; dist.all_gather(ga, a)
assert all(torch.equal(bits(x), bits(ga[0])) for x in ga) and not torch.equal(a, b)
gs = [torch.empty_like(solo[0]) for _ in range(world)]; dist.all_gather(gs, solo[0])
assert all(torch.equal(x, gs[0]) for x in gs)
for bad in (dict(noise=[None] * 7), dict(generator=torch.Generator())):
    try:
        sharded_enhance_batch(m, clips, seed=1, **bad)
    except ValueError as err:
        assert "order" in str(err), err
    else:
        raise AssertionError(f"{list(bad)} was accepted")
assert sharded_enhance_batch(m, [], seed=1) == []
# a CPU all-reduce as the closing barrier: dist.barrier() probes for an accelerator, which opens the GPU on a GPU machine
dist.all_reduce(torch.zeros(1)); dist.destroy_process_group()
print("rank", rank, "ok")
'''


def _port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


@pytest.mark.parametrize("world", [2, 3])
def test_sharded_enhance_batch_gloo(tmp_path, world):
    """7 clips in 3 buckets over 2 and 3 gloo ranks: every rank returns the one-by-one list, bit for bit; each batch of the plan ran on
    exactly one rank; idle ranks take part; seed=None agrees across ranks; noise= / generator= are refused."""
    script = tmp_path / "worker.py"
    script.write_text(_WORKER)
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_port()), WORLD_SIZE=str(world), OMP_NUM_THREADS="1")
    procs = [subprocess.Popen([sys.executable, str(script), ROOT, str(tmp_path)], env=dict(env, RANK=str(r)), stdout=subprocess.PIPE,
                              stderr=subprocess.STDOUT) for r in range(world)]
    outs = [p.communicate(timeout=240)[0].decode() for p in procs]
    assert all(p.returncode == 0 for p in procs), "\n".join(outs)
    assert all("ok" in o for o in outs)
    ran = [tuple(call) for r in range(world) for call in json.loads((tmp_path / f"ran{world}_{r}.json").read_text())]
    assert sorted(ran) == sorted([(1000, 2000), (24575,), (30000, 31000), (50000, 60000)]), ran      # the plan, each batch exactly once


def test_sharded_enhance_batch_without_a_group():
    """World 1 without a process group: still bucketed and batched, no collective; always_gather needs a group."""
    from flowdec_amd.dist import sharded_enhance_batch
    from flowdec_amd.noise import clip_seed

    class FE:
        def _cfg(self):
            return dict(n_fft=1534, hop=384)

    class Stub:
        device = torch.device("cpu"); feature_extractor = FE(); calls = []

        def enhance_batch(self, clips, seeds=None, **kw):
            self.calls.append(len(clips))
            return [c + float(s % 7) for c, s in zip(clips, seeds)]

    clips = [torch.zeros(n) for n in (100, 30000, 200, 300)]
    out = sharded_enhance_batch(Stub(), clips, batch_clips=2, seed=4)
    assert Stub.calls == [2, 1, 1]
    assert all(torch.equal(o, c + float(clip_seed(4, i) % 7)) for i, (o, c) in enumerate(zip(out, clips)))
    with pytest.raises(RuntimeError, match="process group"):
        sharded_enhance_batch(Stub(), clips, seed=4, always_gather=True)
    with pytest.raises(ValueError, match="order"):
        sharded_enhance_batch(Stub(), clips, generator=torch.Generator())


# ------------------------------------------------------------------------------------------------
# enhance_cli --gpus N: what the launcher does without a GPU
# ------------------------------------------------------------------------------------------------
def _argv(tmp_path, *extra):
    return ["--ckpt", str(tmp_path / "none.ckpt"), "--files", str(tmp_path / "in"), "--outdir", str(tmp_path / "out"), "--N", "1", *extra]


@pytest.mark.parametrize("extra,message", [
    (["--gpus", "0"], "at least 1"),
    (["--gpus", "2", "--device", "cuda:1"], "cuda:1"),
    (["--gpus", "9", "--share-gpu"], "at most 8"),
])
def test_cli_gpus_argument_errors(tmp_path, capsys, monkeypatch, extra, message):
    from flowdec_amd import enhance_cli
    monkeypatch.setattr(enhance_cli.subprocess, "Popen", lambda *a, **k: pytest.fail("a process was started"))
    with pytest.raises(SystemExit) as err:
        enhance_cli.run(_argv(tmp_path, *extra))
    assert err.value.code == 2 and message in capsys.readouterr().err


def test_cli_gpus_refuses_a_loaded_model(tmp_path, monkeypatch):
    from flowdec_amd import enhance_cli
    monkeypatch.setattr(enhance_cli.subprocess, "Popen", lambda *a, **k: pytest.fail("a process was started"))
    with pytest.raises(ValueError, match="load --ckpt themselves"):
        enhance_cli.run(_argv(tmp_path, "--gpus", "2", "--share-gpu"), model=object())


def test_cli_gpus_1_is_the_one_process_path(tmp_path, monkeypatch):
    """--gpus 1 (and no flag at all) starts no process: the run happens in the caller's, on the model it was given."""
    from flowdec_amd import enhance_cli
    args = enhance_cli.build_parser().parse_args(_argv(tmp_path))
    assert args.gpus == 1 and not args.share_gpu and args.worker_rank is None and args.worker_manifest is None
    assert "--worker" not in enhance_cli.build_parser().format_help()
    monkeypatch.setattr(enhance_cli.subprocess, "Popen", lambda *a, **k: pytest.fail("a process was started"))
    monkeypatch.setattr(enhance_cli.subprocess, "run", lambda *a, **k: pytest.fail("a process was started"))
    (tmp_path / "in").mkdir()
    from test_cli import synthetic_ckpt
    model = enhance_cli.model_from_checkpoint(synthetic_ckpt())      # on the host: an empty corpus never calls it
    res = enhance_cli.run(_argv(tmp_path, "--gpus", "1", "--rtf"), model=model)
    assert (res.n_done, res.exit_code) == (0, 0)
    assert (tmp_path / "out" / "rtfs.csv").read_text() == "path,runtime,filetime,rtf\n"
    assert sorted(os.listdir(tmp_path / "out")) == ["rtfs.csv"]


def test_manifest_round_trip(tmp_path):
    from flowdec_amd.enhance_cli import FileJob, read_manifest, write_manifest
    jobs = [FileJob(3, "/in/a b.wav", "/out/a b.wav", None, True), FileJob(4, "/in/ü,x.wav", "/out/ü,x.wav", "/clean/ü.wav", False),
            FileJob(7, "in/c.wav", "out/c.wav", "clean/c.wav", True)]
    write_manifest(str(tmp_path / "m.json"), jobs)
    back = read_manifest(str(tmp_path / "m.json"))
    assert back == jobs and [j.index for j in back] == [3, 4, 7] and [j.pending for j in back] == [True, False, True]


def test_merge_parts(tmp_path):
    """Hand-written parts of three ranks with shuffled plan positions -> rtfs.csv in plan order without the position column (rows of one
    position keep their order), the triples list from the work list, the counts summed, exit status 3 kept; the parts are removed."""
    from flowdec_amd.enhance_cli import FileJob, merge_parts, result_part_name, rtf_part_name
    out = tmp_path
    parts = {0: ["4,/o/e.wav,0.5,1.0,0.5", "1,/o/b.wav,0.25,1.0,0.25", "1,/o/a,1.wav,0.25,1.0,0.25"],
             1: ["3,/o/d.wav,0.1,2.0,0.05", "0,/o/c.wav,0.2,2.0,0.1"],
             2: []}
    results = {0: dict(n_done=3, n_over_precision_limit=0, n_too_long=1, gpu_seconds=1.0, audio_seconds=3.0),
               1: dict(n_done=2, n_over_precision_limit=1, n_too_long=0, gpu_seconds=0.3, audio_seconds=4.0),
               2: dict(n_done=0, n_over_precision_limit=0, n_too_long=0, gpu_seconds=0.0, audio_seconds=0.0)}
    for r in range(3):
        (out / rtf_part_name("", r)).write_text("\n".join(["position,path,runtime,filetime,rtf"] + parts[r]) + "\n")
        (out / result_part_name("", r)).write_text(json.dumps(results[r]))
    jobs = [FileJob(0, "/i/x.wav", "/o/x.wav", "/c/x.wav", True), FileJob(1, "/i/y.wav", "/o/y.wav", "/c/y.wav", False)]
    res = merge_parts(str(out), "", 3, jobs, want_rtf=True, want_triples=True)
    assert (out / "rtfs.csv").read_text().splitlines() == ["path,runtime,filetime,rtf", "/o/c.wav,0.2,2.0,0.1", "/o/b.wav,0.25,1.0,0.25",
                                                           "/o/a,1.wav,0.25,1.0,0.25", "/o/d.wav,0.1,2.0,0.05", "/o/e.wav,0.5,1.0,0.5"]
    assert (out / "triples_list.txt").read_text() == "/c/x.wav ---> /i/x.wav ---> /o/x.wav\n/c/y.wav ---> /i/y.wav ---> /o/y.wav\n"
    assert (res.n_done, res.n_over_precision_limit, res.n_too_long, res.exit_code) == (5, 1, 1, 3)
    assert res.gpu_seconds == pytest.approx(1.3) and res.audio_seconds == pytest.approx(7.0)
    assert sorted(os.listdir(out)) == ["rtfs.csv", "triples_list.txt"]
    # no --rtf, no pair list: only the results are read; a suffix names the parts of an --i-min/--i-max window
    (out / result_part_name("_2-5", 0)).write_text(json.dumps(results[2]))
    res = merge_parts(str(out), "_2-5", 1, [], want_rtf=False, want_triples=False)
    assert (res.n_done, res.exit_code) == (0, 0) and sorted(os.listdir(out)) == ["rtfs.csv", "triples_list.txt"]


def test_batch_cost_from_headers(tmp_path):
    """The cost model of the workers' split: files x T_pad, channels x padded frames, channels x rows x row frames, 0 for a header that
    cannot be read and for a file the length rule skips."""
    import argparse
    import numpy as np
    from flowdec_amd import enhance_cli, longform
    from flowdec_amd.enhance_cli import FileJob, batch_cost

    class FE:
        def _cfg(self):
            return dict(n_fft=1534, hop=384)

    class Stub:
        feature_extractor = FE(); sampling_rate = 48000

    def wav(name, n, sr=48000, ch=1):
        enhance_cli.save_wav(str(tmp_path / name), torch.zeros(ch, n), sr)
        return FileJob(0, str(tmp_path / name), str(tmp_path / "o" / name), None, True)

    a, b, st, lo, bad, long_ = wav("a.wav", 30000), wav("b.wav", 12000, 16000), wav("st.wav", 20000, ch=2), wav("lo.wav", 60000), \
        FileJob(0, str(tmp_path / "bad.wav"), "x", None, True), wav("long.wav", 8000 * 3, 8000)
    (tmp_path / "bad.wav").write_bytes(b"RIFF")
    args = argparse.Namespace(chunk_seconds=None, max_seconds=1.5)
    assert batch_cost(Stub(), [a, b], args) == 2 * 128 and batch_cost(Stub(), [a], args) == 128      # b: 36000 samples at 48 kHz
    assert batch_cost(Stub(), [st], args) == 2 * 64 and batch_cost(Stub(), [bad], args) == 0 and batch_cost(Stub(), [long_], args) == 0
    args = argparse.Namespace(chunk_seconds=0.6, max_seconds=1.0)
    rows = len(longform.plan_rows(60000, 384, 64, 16))
    assert rows == 4 and batch_cost(Stub(), [lo], args) == 1 * rows * 64
