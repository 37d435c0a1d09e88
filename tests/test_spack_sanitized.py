"""The member check record's and the sealed pack's host code under
AddressSanitizer + UBSan.  tests/native/spack_fuzz.cpp, a stand-alone program,
feeds fsehip_mcheck_read_header and fsehip_spack_read_header valid, random,
truncated and damaged heads from exact-size heap buffers, and runs the
descriptor planner on random member lists into exact-size arrays, checking
its constants by combining host CRCs the way the kernels do.  fse_mcheck.cpp,
fse_check.cpp, fse_pack.cpp and fse_frame.cpp have no HIP include and build
with g++ alone; nothing is loaded into Python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_spack_heads_and_planner_sanitized(tmp_path):
    exe = tmp_path / "spack_fuzz"
    csrc = os.path.join(ROOT, "entropy_coders_amd", "csrc")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-o", str(exe),
                    os.path.join(ROOT, "tests", "native", "spack_fuzz.cpp"),
                    os.path.join(csrc, "fse_mcheck.cpp"), os.path.join(csrc, "fse_check.cpp"),
                    os.path.join(csrc, "fse_pack.cpp"), os.path.join(csrc, "fse_frame.cpp")],
                   check=True, capture_output=True, timeout=300)
    env = dict(os.environ, ASAN_OPTIONS="verify_asan_link_order=0")
    r = subprocess.run([str(exe), "20000"], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.splitlines()
    assert len(lines) == 2 and lines[0].startswith("ok heads") and lines[1].startswith("ok planner"), r.stdout
