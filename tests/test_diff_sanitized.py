"""The diff frame's host code under AddressSanitizer + UBSan.
tests/native/diff_fuzz.cpp, a stand-alone program, feeds
fsehip_diff_read_header valid, random, truncated and bit-flipped 48-byte heads
from exact-size heap buffers, and random range lists to the range-scratch
formula and the range checks of the new kind
(entropy_coders_amd/csrc/fse_elem.cpp and fse_frame.cpp have no HIP include
and build with g++ alone): every header result is FSE_OK with its fields in
range, or BAD_FRAME; every range result equals a 128-bit restatement."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_diff_header_and_ranges_sanitized(tmp_path):
    exe = tmp_path / "diff_fuzz"
    csrc = os.path.join(ROOT, "entropy_coders_amd", "csrc")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-o", str(exe),
                    os.path.join(ROOT, "tests", "native", "diff_fuzz.cpp"),
                    os.path.join(csrc, "fse_elem.cpp"), os.path.join(csrc, "fse_frame.cpp")],
                   check=True, capture_output=True, timeout=300)
    r = subprocess.run([str(exe), "20000"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.startswith("ok"), r.stdout
