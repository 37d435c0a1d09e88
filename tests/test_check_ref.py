"""The check record's reference (tests/check_ref.py) against zlib, no GPU: the
written-out combine equals zlib.crc32 of the concatenation, and records have
the stated sizes and a content_crc equal to zlib.crc32."""
import zlib

import numpy as np
import pytest

import check_ref as K
from entropy_coders_amd import _lib


def test_the_library_has_the_check_calls():
    lib = _lib.load()
    for name in ("fsehip_check_build", "fsehip_check_verify", "fsehip_check_verify_ranges", "fsehip_crc32",
                 "fsehip_sealed_read_header"):
        assert getattr(lib, name) is not None
    assert _lib.STATUS[-21] == "CHECKSUM"


def test_combine_equals_the_crc_of_the_concatenation():
    rng = np.random.default_rng(0xC4C)
    lens = [0, 1, 2, 255, 256, 4097]
    pairs = [(a, b) for a in (0, 1) for b in (0, 1)] + [(int(rng.choice(lens)), int(rng.integers(0, 3000)))
                                                         for _ in range(200)]
    for la, lb in pairs:
        a, b = rng.integers(0, 256, la, dtype=np.uint8).tobytes(), rng.integers(0, 256, lb, dtype=np.uint8).tobytes()
        assert K.combine(zlib.crc32(a), zlib.crc32(b), lb) == zlib.crc32(a + b), (la, lb)
        assert K.combine(zlib.crc32(b), zlib.crc32(a), la) == zlib.crc32(b + a), (lb, la)


@pytest.mark.parametrize("check_log", [8, 12, 16])
def test_records(check_log):
    B = 1 << check_log
    rng = np.random.default_rng(check_log)
    for n in (0, 1, B - 1, B, B + 1, 3 * B + 5):
        content = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        rec = K.record(content, check_log)
        f = K.parse(rec)
        assert len(rec) == K.record_bytes(n, check_log) == 32 + 4 * ((n + B - 1) // B)
        assert f["content_crc"] == (zlib.crc32(content) if n else 0) and f["n_content"] == n
        assert f["header_crc"] == zlib.crc32(rec[:28])
        assert f["table"] == [zlib.crc32(content[i: i + B]) for i in range(0, n, B)]


def test_covered_blocks_by_hand():
    assert K.covered(1000, 8, 0, 1000) == [0, 1, 2, 3]
    assert K.covered(1000, 8, 1, 999) == [1, 2, 3]         # the ragged last block counts: the range ends at n
    assert K.covered(1000, 8, 0, 999) == [0, 1, 2]
    assert K.covered(1000, 8, 256, 256) == [1]
    assert K.covered(1000, 8, 255, 258) == [1]
    assert K.covered(1000, 8, 257, 255) == []
    assert K.covered(1000, 8, 1000, 0) == [] and K.covered(1024, 8, 768, 0) == []
    assert K.verified_bytes(1000, 8, [(1, 999, 0), (0, 256, 0)]) == 744 + 256
