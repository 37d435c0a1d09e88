"""The host code of the estimate with a base under AddressSanitizer + UBSan.
tests/native/estimate_diff_fuzz.cpp, a stand-alone program, builds
entropy_coders_amd/csrc/fse_estimate.cpp alone (no HIP include, g++ only) and
holds fsehip_estimate_choose_base against the tie rule written out again, on
exact-size heap buffers, and fsehip_estimate_base_scratch_bytes against its
formula in 128-bit integers, on random and degenerate inputs."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_estimate_diff_host_sanitized(tmp_path):
    exe = tmp_path / "estimate_diff_fuzz"
    csrc = os.path.join(ROOT, "entropy_coders_amd", "csrc")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-o", str(exe),
                    os.path.join(ROOT, "tests", "native", "estimate_diff_fuzz.cpp"),
                    os.path.join(csrc, "fse_estimate.cpp")],
                   check=True, capture_output=True, timeout=300)
    env = dict(os.environ, ASAN_OPTIONS="verify_asan_link_order=0")
    r = subprocess.run([str(exe), "20000"], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.startswith("ok"), r.stdout
