"""The pack frame's host code under AddressSanitizer + UBSan.
tests/native/pack_fuzz.cpp, a stand-alone program, feeds
fsehip_pack_read_header and fsehip_pack_read_members valid, random, truncated
and damaged heads, truncated tables, member counts beyond the buffer and
counts whose sums overflow, from exact-size heap buffers into exact-size
member arrays, and runs the planner on what is accepted, with random
selections (entropy_coders_amd/csrc/fse_pack.cpp and fse_frame.cpp have no HIP
include and build with g++ alone): every result is FSE_OK with its fields in
range, or BAD_FRAME."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_pack_head_and_planner_sanitized(tmp_path):
    exe = tmp_path / "pack_fuzz"
    csrc = os.path.join(ROOT, "entropy_coders_amd", "csrc")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-o", str(exe),
                    os.path.join(ROOT, "tests", "native", "pack_fuzz.cpp"),
                    os.path.join(csrc, "fse_pack.cpp"), os.path.join(csrc, "fse_frame.cpp")],
                   check=True, capture_output=True, timeout=300)
    env = dict(os.environ, ASAN_OPTIONS="verify_asan_link_order=0")
    r = subprocess.run([str(exe), "20000"], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.startswith("ok"), r.stdout
