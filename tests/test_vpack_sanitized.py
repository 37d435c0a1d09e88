"""The versioned pack's host code under AddressSanitizer + UBSan.
tests/native/vpack_fuzz.cpp, a stand-alone program, feeds the readers of both
containers that entropy_coders_amd/csrc/fse_pack.cpp implements (the pack
frame's and the versioned pack's) valid, random, truncated and damaged heads
from exact-size heap buffers into exact-size member arrays, runs the planner
on what is accepted, and checks the device calls' pointer rules (the bases,
and the decode side's overlap check with its in-place exception) against a
pair-by-pair restatement on random layouts.  fse_pack.cpp and fse_frame.cpp
have no HIP include and build with g++ alone; nothing is loaded into Python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_vpack_heads_planner_and_pointer_checks_sanitized(tmp_path):
    exe = tmp_path / "vpack_fuzz"
    csrc = os.path.join(ROOT, "entropy_coders_amd", "csrc")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-o", str(exe),
                    os.path.join(ROOT, "tests", "native", "vpack_fuzz.cpp"),
                    os.path.join(csrc, "fse_pack.cpp"), os.path.join(csrc, "fse_frame.cpp")],
                   check=True, capture_output=True, timeout=300)
    env = dict(os.environ, ASAN_OPTIONS="verify_asan_link_order=0")
    r = subprocess.run([str(exe), "20000"], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.splitlines()
    assert len(lines) == 2 and lines[0].startswith("ok heads") and lines[1].startswith("ok spans"), r.stdout
