"""The host-only logic of the native model code, tested without a GPU: the workspace planner (flowdec_amd/csrc/arena.h) and the solvers'
time grids, NFE counts and adaptive step-size controller (flowdec_amd/csrc/step_ctl.h).

Both headers compile with a plain C++ compiler.  The programs under tests/c include them directly, have their own main, and are built twice
with g++ -std=c++17: plain, and with -fsanitize=address,undefined -fno-sanitize-recover=all.  They run as stand-alone executables; a
violated property or a sanitizer report is a non-zero exit status."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from oracle import flowdec_oracle as O

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
BUILDS = {"plain": [], "sanitized": SANITIZE}

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")


@pytest.fixture(scope="module", params=sorted(BUILDS))
def programs(request, tmp_path_factory):
    """{name: executable} of tests/c/arena_check.cpp and step_ctl_check.cpp in one of the two builds."""
    d = tmp_path_factory.mktemp("host_" + request.param)
    out = {}
    for name in ("arena_check", "step_ctl_check"):
        out[name] = str(d / name)
        subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", *BUILDS[request.param], "-I", os.path.join(ROOT, "flowdec_amd", "csrc"),
                        "-I", os.path.join(ROOT, "include"), os.path.join(HERE, "c", name + ".cpp"), "-o", out[name]], check=True)
    return out


def run(exe, *args):
    r = subprocess.run([exe, *[repr(a) if isinstance(a, float) else str(a) for a in args]], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    return r.stdout.splitlines()


def test_arena_random_histories(programs):
    """2000 random alloc / release histories of 400 operations and two ordered ones: aligned offsets, no overlap of live blocks, peak() =
    the largest end handed out, after every operation; an emptied arena starts at 0 again."""
    assert run(programs["arena_check"])[-1].startswith("arena ok")


def fields(line):
    """'end accept 1 landed 0 t 0x1p-2 dt 0x1p-3' -> {'accept': '1', ...} (values stay text: %a floats are compared as bit patterns)"""
    tok = line.split()
    return dict(zip(tok[1::2], tok[2::2]))


def test_step_ctl_traces(programs):
    """One StepCtl driven as the adaptive solvers drive it gives the recorded trace, line for line (every float as %a) -- and the recorded
    traces are live: each ends at ts[N] exactly, lands its N checkpoints in order, and has rejected and accepted attempts."""
    with open(os.path.join(HERE, "golden", "step_ctl_traces.json")) as f:
        golden = json.load(f)
    assert "5771fb5" in golden["source"]
    assert len(golden["scenarios"]) == 10
    for s in golden["scenarios"]:
        lines, N = s["lines"], s["args"][1]
        ts = lines[0].split()[1:]
        ends = [fields(l) for l in lines if l.startswith("end ")]
        assert len(ts) == N + 1 and lines[-1].startswith("done ") and len(ends) == int(fields(lines[-1])["attempts"]) < 10000, s["name"]
        assert fields(lines[-1])["t"] == ends[-1]["t"] == ts[N], f"{s['name']}: does not end at ts[N] bit for bit"
        assert [int(e["landed"]) for e in ends if e["landed"] != "0"] == list(range(1, N + 1)), f"{s['name']}: checkpoints not landed in order"
        assert all(e["accept"] == "1" for e in ends if e["landed"] != "0")
        accepts = {e["accept"] for e in ends}
        assert accepts == ({"1"} if s["only_accepts"] else {"0", "1"}), f"{s['name']}: accepts / rejects {accepts}"
        assert run(programs["step_ctl_check"], "trace", *s["args"]) == lines, f"{s['name']}: the controller's trace moved"


def test_time_grids_and_nfe_equal_the_oracle(programs):
    """t_span_linspace(N) and linspace_f32(1, 0.03, N) bit for bit against the oracle's functions of the same names, N = 1..64; solver_nfe
    for the four solver ids and an unknown one."""
    f32 = lambda toks: np.array([float.fromhex(t) for t in toks], dtype=np.float64).astype(np.float32)
    rows = {}
    for line in run(programs["step_ctl_check"], "grids", 64, 1.0, 0.03):
        kind, N, *vals = line.split()
        rows[kind, int(N)] = vals
    assert len(rows) == 3 * 64
    for N in range(1, 65):
        for kind, ref in (("t_span", O.t_span_linspace(N)), ("linspace", O.linspace_f32(1.0, 0.03, N))):
            got = f32(rows[kind, N])
            assert ref.dtype == np.float32 and got.shape == ref.shape and np.array_equal(got.view(np.uint32), ref.view(np.uint32)), (kind, N)
        want = [O.solver_nfe(s, N) for s in ("euler", "midpoint", "heun2", "heun2_eulerlast")] + [-1]
        assert [int(v) for v in rows["nfe", N]] == want == [N, 2 * N, 2 * N, 2 * N - 1, -1], N
