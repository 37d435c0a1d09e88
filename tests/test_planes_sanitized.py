"""The plane frame's host code under AddressSanitizer + UBSan.
tests/native/planes_fuzz.cpp, a stand-alone program, feeds
fsehip_planes_read_header valid, random, truncated and bit-flipped 48-byte
heads from exact-size heap buffers (entropy_coders_amd/csrc/fse_elem.cpp and
fse_frame.cpp have no HIP include and build with g++ alone): every result is
FSE_OK with its fields in range, or BAD_FRAME."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_planes_header_sanitized(tmp_path):
    exe = tmp_path / "planes_fuzz"
    csrc = os.path.join(ROOT, "entropy_coders_amd", "csrc")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-o", str(exe),
                    os.path.join(ROOT, "tests", "native", "planes_fuzz.cpp"),
                    os.path.join(csrc, "fse_elem.cpp"), os.path.join(csrc, "fse_frame.cpp")],
                   check=True, capture_output=True, timeout=300)
    env = dict(os.environ, ASAN_OPTIONS="verify_asan_link_order=0")
    r = subprocess.run([str(exe), "20000"], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.startswith("ok"), r.stdout
