"""The layering of the package's Python: _lib -> ops, noise, longform, audio, batching -> resample, metrics, align, estimate, loss ->
specdist, segsnr, loudness -> model -> checkpoint, dist, stream -> the five *_cli.  No library module imports a command line, the
function-local intra-package imports that remain are listed here with their reasons, the measurement modules take nothing private from a
sibling, and the pieces the layers share -- `batching.padded_rows` (clips -> zero-padded rows), `batching.plan_clip_batches` (the T_pad
bucket plan) and `batching.ragged_batches` (the loop over length-sorted batches) -- are each one function."""
import ast
import glob
import os
import subprocess
import sys

import pytest
import torch

from conftest import ROOT

LIBRARY_MODULES = ("audio", "batching", "checkpoint", "resample", "metrics", "estimate", "loss", "dist", "stream", "longform", "noise", "ops", "model",
                   "align", "specdist", "segsnr", "loudness")
MEASUREMENT_MODULES = ("metrics", "align", "specdist", "segsnr", "loudness")

# (file, imported module) -> why the import stays inside a function
LAZY_IMPORTS = {
    ("audio.py", "resample"): "a true cycle: resample.py takes the filter bank (sinc_resample_kernel) from audio at module level",
    ("boxprobe.py", "_lib"): "the power sampler of boxprobe runs without torch and without the library; only calibrate() needs them",
}


def test_no_library_module_imports_a_command_line():
    code = ("import importlib, sys, torch\n"
            f"for m in {LIBRARY_MODULES!r}:\n"
            "    importlib.import_module('flowdec_amd.' + m)\n"
            "import flowdec_amd._lib as L\n"
            "print(sorted(k for k in sys.modules if k.startswith('flowdec_amd.') and k.endswith('_cli')))\n"
            "print(L._lib is None, torch.cuda.is_initialized())\n")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.strip().splitlines()
    assert lines[-2] == "[]", f"library modules pulled in a command line: {lines[-2]}"
    assert lines[-1] == "True False", "importing the library modules loaded the .so or initialised the GPU"


def test_lazy_intra_package_imports_are_the_listed_ones():
    found = set()
    for path in sorted(glob.glob(os.path.join(ROOT, "flowdec_amd", "*.py"))):
        with open(path, "r") as f:
            tree = ast.parse(f.read(), path)
        for fn in ast.walk(tree):
            if not isinstance(fn, (ast.FunctionDef, ast.AsyncFunctionDef, ast.Lambda)):
                continue
            for node in ast.walk(fn):
                if isinstance(node, ast.ImportFrom) and node.level >= 1:
                    for target in ([node.module] if node.module else [a.name for a in node.names]):
                        found.add((os.path.basename(path), target.split(".")[0]))
    assert len(LAZY_IMPORTS) <= 4 and all(isinstance(why, str) and why for why in LAZY_IMPORTS.values())
    assert found <= set(LAZY_IMPORTS), f"function-local intra-package imports outside the allow-list: {sorted(found - set(LAZY_IMPORTS))}"


def test_measurement_modules_take_nothing_private_from_a_sibling():
    """None of MEASUREMENT_MODULES imports an underscore-prefixed name from another module of the package or reads one through a module
    alias (`metrics._x`); `_lib` itself, the lowest layer, is the one module they may name.  And the loop over length-sorted batches
    exists once in the package."""
    siblings = {os.path.splitext(os.path.basename(p))[0] for p in glob.glob(os.path.join(ROOT, "flowdec_amd", "*.py"))}
    found, loops = [], []
    for path in sorted(glob.glob(os.path.join(ROOT, "flowdec_amd", "*.py"))):
        name = os.path.splitext(os.path.basename(path))[0]
        with open(path, "r") as f:
            src = f.read()
        loops += [name] * src.count("for idx in length_sorted_batches")
        if name not in MEASUREMENT_MODULES:
            continue
        tree = ast.parse(src, path)
        aliases = {}                                            # local name -> sibling module it stands for
        for node in ast.walk(tree):
            if isinstance(node, ast.ImportFrom) and node.level >= 1:
                for a in node.names:
                    if node.module is None and a.name in siblings:
                        aliases[a.asname or a.name] = a.name    # from . import metrics [as m]
                    if node.module is not None and a.name.startswith("_"):
                        found.append(f"{name}: from .{node.module} import {a.name}")
        for node in ast.walk(tree):
            if (isinstance(node, ast.Attribute) and isinstance(node.value, ast.Name) and node.value.id in aliases
                    and aliases[node.value.id] != "_lib" and node.attr.startswith("_")):
                found.append(f"{name}: {node.value.id}.{node.attr}")
    assert not found, found
    assert loops == ["batching"], loops


def _clips(lengths):
    return [torch.arange(1, n + 1, dtype=torch.float32) * (k + 1) for k, n in enumerate(lengths)]


def _check_rows(rows, lens, clips, Lrow):
    assert rows.dtype == torch.float32 and rows.shape == (len(clips), Lrow)
    assert lens.dtype == torch.int32 and lens.tolist() == [c.numel() for c in clips]
    for b, c in enumerate(clips):
        assert torch.equal(rows[b, :c.numel()], c)
        assert torch.equal(rows[b, c.numel():], torch.zeros(Lrow - c.numel()))      # exactly 0.0 behind the clip


@pytest.mark.parametrize("Lrow", [17, 23])
def test_padded_rows_on_the_host(Lrow):
    from flowdec_amd.batching import padded_rows
    clips = _clips([1, 5, 17])
    rows, lens = padded_rows(clips, Lrow, "cpu")
    _check_rows(rows, lens, clips, Lrow)
    buf = torch.full((3, Lrow), float("nan"))
    rows, lens = padded_rows(clips, Lrow, "cpu", out=buf)
    assert rows.data_ptr() == buf.data_ptr()
    _check_rows(buf, lens, clips, Lrow)
    with pytest.raises(ValueError):
        padded_rows(_clips([1, Lrow + 1]), Lrow, "cpu")


@pytest.mark.parametrize("batch_files", [1, 3, 8])
def test_plan_clip_batches_is_the_one_planner(tmp_path, batch_files):
    """enhance_cli.plan_batches on wav headers = batching.plan_clip_batches on their lengths: the same index groups in the same order
    (ascending T_pad, then clip order -- the row order of rtfs.csv)."""
    from types import SimpleNamespace
    import flowdec_amd.batching as batching
    import flowdec_amd.dist as dist
    from flowdec_amd import enhance_cli
    from flowdec_amd.audio import save_wav
    assert dist.plan_clip_batches is batching.plan_clip_batches
    hop = 384
    base = [24575, 24576, 49152, 24000, 49000, 24576, 12000, 49151, 30000, 24575]       # T_pad 64 up to 24575 samples, 128 up to 49151, then 192
    lengths = base + [n - 7 * k for k, n in enumerate(base)]
    assert len(lengths) == 20 and len({batching.padded_frames_of(n, hop) for n in lengths}) == 3
    jobs = []
    for i, n in enumerate(lengths):
        src = str(tmp_path / f"c{i:02d}.wav")
        save_wav(src, torch.zeros(n), 48000)
        jobs.append(enhance_cli.FileJob(i, src, src + ".out", None, True))
    model = SimpleNamespace(sampling_rate=48000, feature_extractor=SimpleNamespace(_cfg=lambda: dict(hop=hop)))
    got = [[j.index for j in batch] for batch in enhance_cli.plan_batches(model, jobs, batch_files)]
    want = [idx for _, idx in batching.plan_clip_batches(lengths, hop, batch_files)] if batch_files > 1 else [[i] for i in range(20)]
    assert got == want
    plan = batching.plan_clip_batches(lengths, hop, batch_files)
    assert [tp for tp, _ in plan] == sorted(tp for tp, _ in plan) and sorted(i for _, idx in plan for i in idx) == list(range(20))
    assert all(len(idx) <= batch_files and idx == sorted(idx) for _, idx in plan)


@pytest.mark.gpu
def test_padded_rows_mixed_residency():
    """A clip that already lives on the GPU among host clips: the same rows and lengths as from host clips alone, also through out=."""
    from flowdec_amd.batching import padded_rows
    clips = _clips([5, 17, 9])
    want_rows, want_lens = padded_rows(clips, 23, "cpu")
    mixed = [clips[0], clips[1].to("cuda"), clips[2]]
    rows, lens = padded_rows(mixed, 23, "cuda")
    assert rows.is_cuda and lens.is_cuda and torch.equal(rows.cpu(), want_rows) and torch.equal(lens.cpu(), want_lens)
    buf = torch.full((3, 23), float("nan"), device="cuda")
    rows, lens = padded_rows(mixed, 23, "cuda", out=buf)
    assert rows.data_ptr() == buf.data_ptr() and torch.equal(buf.cpu(), want_rows) and torch.equal(lens.cpu(), want_lens)
    rows, lens = padded_rows(clips, 23, "cuda", out=buf.fill_(float("nan")))      # host clips: one block, one copy
    assert torch.equal(buf.cpu(), want_rows) and torch.equal(lens.cpu(), want_lens)
