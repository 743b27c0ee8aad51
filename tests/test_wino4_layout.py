"""The layout arithmetic of the F(4,3) bf16 kernel's producer pass (flowdec_amd/csrc/wino4_layout.h), checked exhaustively on the host.

tests/wino4_layout_check.cpp includes the header the kernel includes and walks every lane of every LDS instruction of the pass: bank
conflicts of the RAW reads and V stores, every (pixel, piece) of the halo requested exactly once, every V word of a chunk written
exactly once.  It is compiled as a stand-alone program with AddressSanitizer and UndefinedBehaviorSanitizer and run as such."""
import os
import shutil
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def _compiler():
    for c in (os.environ.get("CXX"), "c++", "g++", "clang++", "/opt/rocm/llvm/bin/clang++"):
        if c and shutil.which(c):
            return shutil.which(c)
    raise RuntimeError("no host C++ compiler found (set CXX)")


def test_layout_check_under_sanitizers(tmp_path):
    exe = str(tmp_path / "wino4_layout_check")
    cmd = [_compiler(), "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", os.path.join(ROOT, "flowdec_amd", "csrc"), os.path.join(HERE, "wino4_layout_check.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, "compile failed:\n" + r.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "wino4_layout_check: OK" in r.stdout, r.stdout[-4000:] + r.stderr[-4000:]
