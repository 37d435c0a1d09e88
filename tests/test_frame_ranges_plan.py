"""The host planner of fsehip_frame_decompress_ranges under AddressSanitizer
+ UBSan.  tests/native/frame_ranges_fuzz.cpp checks
fsehip::frame_plan_ranges (entropy_coders_amd/csrc/fse_frame.cpp, no HIP
include: built with g++ alone) against a brute-force per-byte model on seeded
random headers and range sets: every (range, byte) served by exactly one
piece inside its block, the unique block list sorted and complete, direct
runs whole blocks with aligned destinations, chunks within chunk_blocks with
the short last block last, and the call's rejections."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_range_planner_sanitized(tmp_path):
    exe = tmp_path / "frame_ranges_fuzz"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-o", str(exe),
                    os.path.join(ROOT, "tests", "native", "frame_ranges_fuzz.cpp"),
                    os.path.join(ROOT, "entropy_coders_amd", "csrc", "fse_frame.cpp")],
                   check=True, capture_output=True, timeout=300)
    env = dict(os.environ, ASAN_OPTIONS="verify_asan_link_order=0")
    r = subprocess.run([str(exe), "20000"], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert r.stdout.startswith("ok 20000"), r.stdout


def test_header_declares_the_range_calls():
    """The export side is tests/test_abi.py's (every name of _lib.EXPORTS is
    declared and exported); here: the new names are among them, with the
    documented struct."""
    from entropy_coders_amd import _lib

    text = open(os.path.join(ROOT, "include", "fsehip.h")).read()
    for name in ("fsehip_frame_decompress_ranges", "fsehip_frame_decompress_range"):
        assert name in _lib.EXPORTS
        assert re.search(r"\bint\s+%s\s*\(" % name, text), name
    body = re.search(r"typedef struct \{([^}]*)\}\s*fsehip_frame_range;", text)
    assert body, "fsehip_frame_range is not declared"
    fields = re.findall(r"uint64_t\s+(\w+);", body.group(1))
    assert fields == ["src_off", "len", "dst_off"] == [f for f, _ in _lib.FrameRange._fields_]
    import entropy_coders_amd as E

    assert "frame_decompress_range" in E.__all__
    for method in ("decompress_frame_ranges_into", "decompress_frame_ranges", "decompress_frame_range"):
        assert callable(getattr(E.BlockCodec, method))
