#!/usr/bin/env python
"""tests/golden/step_ctl_traces.json: what one StepCtl (flowdec_amd/csrc/step_ctl.h) does on fixed scenarios, every float as %a.

The fixture pins the controller's ROUNDINGS (float / double casts, order of operations), on which accept / reject rests, against later
edits of the header.  Generate it only from a header whose text is the one to pin -- SOURCE below names it -- never from a header edited
since: builds tests/c/step_ctl_check.cpp with g++ and records its `trace` output per scenario.

    python tests/golden/make_golden_step_ctl.py
"""
import json
import os
import subprocess
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
SOURCE = ("StepCtl, the tableaux and t_span_linspace as moved verbatim into flowdec_amd/csrc/step_ctl.h from flowdec_amd/csrc/model.hip of "
          "commit 5771fb5 (\"Layer the host Python: audio, checkpoint and batching modules\"), before any other edit")
METHODS = {"dopri5": 0, "tsit5": 1}
# accept below 1 (factor floor 1), reject (factor in (0.2, 1)), ratio == 0, the accept boundary 1.0, the cap 10, the floor 0.2, accept near 1
RATIOS = [0.5, 1.5, 0.0, 1.0, 1e-12, 1e6, 0.9]


def scenarios():
    out = []
    for name, mid in METHODS.items():
        for N in (1, 3, 4):    # N > 1: checkpoint-shortened steps and their dt_old - dt restore; every N: the final clamp to ts[N]
            out.append({"name": f"{name}_N{N}", "args": [mid, N, 0.125, 0.5, 0.25] + RATIOS, "only_accepts": False})
        out.append({"name": f"{name}_tiny_d0", "args": [mid, 3, 1e-6, 0.5, 0.25] + RATIOS, "only_accepts": False})   # probe_step's 1e-6 branch
        # first_step's fallback max(1e-6, 1e-3 h0), then growth by 10 per attempt
        out.append({"name": f"{name}_flat", "args": [mid, 3, 0.125, 0.0, 0.0, 0.0], "only_accepts": True})
    return out


def main():
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "step_ctl_check")
        subprocess.run(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "flowdec_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "c", "step_ctl_check.cpp"), "-o", exe], check=True)
        sc = scenarios()
        for s in sc:
            r = subprocess.run([exe, "trace"] + [repr(a) for a in s["args"]], capture_output=True, text=True, check=True)
            s["lines"] = r.stdout.splitlines()
    with open(os.path.join(HERE, "step_ctl_traces.json"), "w") as f:
        json.dump({"source": SOURCE, "scenarios": sc}, f, indent=1)
        f.write("\n")
    print("wrote", len(sc), "scenarios,", sum(len(s["lines"]) for s in sc), "lines")


if __name__ == "__main__":
    main()
