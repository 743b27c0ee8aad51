"""The host-only logic of the native model code, tested without a GPU: the workspace planner (flowdec_amd/csrc/arena.h), the solvers'
time grids, NFE counts and adaptive step-size controller (flowdec_amd/csrc/step_ctl.h), and the NDAC codec's structure -- parameter table,
layer records, lengths, workspace, halos (flowdec_amd/csrc/ndac_plan.h).

The headers compile with a plain C++ compiler.  The programs under tests/c include them directly, have their own main, and are built twice
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
    """{name: executable} of tests/c/arena_check.cpp, step_ctl_check.cpp and ndac_plan_check.cpp in one of the two builds."""
    d = tmp_path_factory.mktemp("host_" + request.param)
    out = {}
    for name in ("arena_check", "step_ctl_check", "ndac_plan_check"):
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


# ---- the NDAC codec's plan (flowdec_amd/csrc/ndac_plan.h) ----------------------------------------------------------------------------------
def _ndac_configs():
    from test_ndac_cpu import NDAC75_LIKE, SMALL
    return {"small": SMALL, "ndac75_like": NDAC75_LIKE, "small_enc32": dict(SMALL, encoder_dim=32),
            "one_rate": dict(SMALL, encoder_rates=(3,), decoder_rates=(2,))}


# the decode halo of SMALL is the plan's own arithmetic: fd_ndac_decode_halo refuses its odd rate 5
NDAC_HALOS = {"small": ((13, 13), (15, 15)), "ndac75_like": ((7, 7), (9, 9)), "small_enc32": ((13, 13), (15, 15)), "one_rate": ((16, 16), (25, 25))}


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from flowdec_amd import _lib
    return _lib.load()


@pytest.mark.parametrize("name", ["small", "ndac75_like", "small_enc32", "one_rate"])
def test_ndac_plan_against_the_module_tree_the_oracle_and_the_parent(programs, lib, name):
    """The plan's parameter table is the module's effective state_dict; its layer records are the module tree's convolutions in order; its
    lengths are the oracle's; the workspace fd_ndac_workspace_bytes derives from it is, byte for byte, what the library returned before the
    plan existed (tests/golden/ndac_workspace_bytes.json, recorded from that build); the halos are the values the rules gave then."""
    import ctypes as C
    import torch
    from flowdec_amd.ndac import DAC
    from oracle import ndac_oracle as N
    from test_ndac_cpu import native_codec, scaled_sd
    cfg = _ndac_configs()[name]
    dac = DAC(**cfg)
    hop, frames = dac.hop_length, (1, 2, 7)
    args = [cfg["encoder_dim"], ",".join(map(str, cfg["encoder_rates"])), dac.latent_dim, cfg["decoder_dim"], ",".join(map(str, cfg["decoder_rates"])),
            cfg["n_codebooks"], cfg["codebook_size"], cfg["codebook_dim"]]
    for n in (1, 2, 3, 7):
        args += ["len", n * hop, "slot", n * hop]
    for T in frames:
        args += ["frames", T]
    rows = [l.split() for l in run(programs["ndac_plan_check"], *args)]
    # (1) the parameter table
    params = {r[1]: tuple(int(v) for v in r[2:]) for r in rows if r[0] == "param"}
    eff = {k: tuple(v.shape) for k, v in dac._effective().items()}
    assert params == eff and len(params) == sum(r[0] == "param" for r in rows)
    # (2) lengths
    lens = {int(r[1]): int(r[2]) for r in rows if r[0] == "len"}
    assert [lens[n * hop] for n in (1, 2, 3)] == [1, 2, 3] and int([r for r in rows if r[0] == "hop"][0][1]) == hop
    o = N.DACOracle(scaled_sd(cfg, 3, 0.7), **cfg)
    decoded = {int(r[1]): int(r[2]) for r in rows if r[0] == "frames"}
    for T in frames:
        assert decoded[T] == o.decode(np.zeros((1, o.cfg["latent_dim"], T), np.float32)).shape[-1], T
    # (3) one record per convolution of the module tree, in order
    for tag, tree in (("enc", dac.encoder), ("dec", dac.decoder)):
        convs = [m for m in tree.modules() if isinstance(m, (torch.nn.Conv1d, torch.nn.ConvTranspose1d))]
        recs = [r for r in rows if r[0] == tag]
        assert len(recs) == len(convs)
        for r, m in zip(recs, convs):
            assert r[1] == ("convT" if isinstance(m, torch.nn.ConvTranspose1d) else "conv")
            assert [int(v) for v in r[2:8]] == [m.in_channels, m.out_channels, m.kernel_size[0], m.stride[0], m.padding[0], m.dilation[0]], r
            assert params[r[8]] == tuple(m.weight.shape) and params[r[9]] == (m.out_channels,) and r[8][:-len("weight")] == r[9][:-len("bias")]
        # residual adds and raw outputs: a ResidualUnit is (7-tap: nothing raw; 1x1: adds the unit's input), raw kept where another unit follows
        unit = lambda raw: [("0", "0"), ("1", raw)]
        n_rates = len(cfg[("encoder" if tag == "enc" else "decoder") + "_rates"])
        want = [("0", "1" if tag == "enc" else "0")]
        for i in range(n_rates):
            if tag == "enc":
                want += unit("1") + unit("1") + unit("0") + [("0", "0" if i + 1 == n_rates else "1")]
            else:
                want += [("0", "1")] + unit("1") + unit("1") + unit("0")
        want += [("0", "1")]
        assert [(r[11], r[12]) for r in recs] == want
        assert [r[13] for r in recs] == ["0"] * (len(recs) - 1) + ["1" if tag == "dec" else "0"]
        assert all((r[10] == "-") == (i + 1 == len(recs)) for i, r in enumerate(recs))      # every layer but a stack's last feeds a Snake
    # (4) the workspace, against the build before the plan
    with open(os.path.join(HERE, "golden", "ndac_workspace_bytes.json")) as f:
        golden = json.load(f)
    assert "e828d71" in golden["source"]
    slots = {int(r[1]): int(r[2]) for r in rows if r[0] == "slot"}
    h = native_codec(lib, cfg)
    try:
        lib.fd_ndac_workspace_bytes.restype = C.c_size_t
        assert lib.fd_ndac_num_params(h) == len(params)
        for B in (1, 3):
            for n in (1, 7):
                got = lib.fd_ndac_workspace_bytes(h, B, n * hop)
                assert got == golden["workspace_bytes"][name][f"B{B}_L{n}hop"], (B, n, got)
                assert 0 <= (got - 256) // 5 - 4 * B * slots[n * hop] < 256          # five slots of the plan's widest tensor, 256-byte aligned
    finally:
        lib.fd_ndac_destroy(h)
    # the halos and their preconditions
    facts = {r[0]: r[1:] for r in rows}
    assert (tuple(map(int, facts["encode_halo"])), tuple(map(int, facts["decode_halo"]))) == NDAC_HALOS[name]
    assert facts["whole_frames"] == ["ok"] and (facts["even_rates"] == ["ok"]) == all(s % 2 == 0 for s in cfg["decoder_rates"])


def test_ndac_plan_preconditions(programs):
    """A rate of 1 and rates that do not give whole frames are named; so is an odd decoder rate."""
    base = [8, None, 64, 64, None, 2, 32, 8]
    facts = lambda er, dr: {l.split()[0]: l.split(None, 1)[1] for l in run(programs["ndac_plan_check"], *[er if i == 1 else dr if i == 4 else v for i, v in enumerate(base)])
                            if l.split()[0] in ("whole_frames", "even_rates", "hop", "up")}
    f = facts("2,1,4", "4,5")
    assert "rate of 1" in f["whole_frames"] and "decoder rate 5 is odd" in f["even_rates"] and (f["hop"], f["up"]) == ("8", "20")
    assert facts("2,4,8,8", "8,8,4,2") == {"whole_frames": "ok", "even_rates": "ok", "hop": "512", "up": "512"}
