"""The check record's host code under AddressSanitizer + UBSan.
tests/native/check_fuzz.cpp, a stand-alone program built with g++ from
entropy_coders_amd/csrc/fse_check.cpp alone (no HIP include), feeds the header
readers valid, random, truncated and bit-flipped heads from exact-size heap
buffers, runs the host CRC-32 at every alignment and at lengths 0..70 against
a bitwise CRC written in the program, the combine against the CRC of the
concatenation, and the range planner against a per-byte model."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_check_host_code_sanitized(tmp_path):
    exe = tmp_path / "check_fuzz"
    csrc = os.path.join(ROOT, "entropy_coders_amd", "csrc")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-o", str(exe),
                    os.path.join(ROOT, "tests", "native", "check_fuzz.cpp"), os.path.join(csrc, "fse_check.cpp")],
                   check=True, capture_output=True, timeout=300)
    env = dict(os.environ, ASAN_OPTIONS="verify_asan_link_order=0")
    r = subprocess.run([str(exe), "20000"], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.startswith("ok"), r.stdout
