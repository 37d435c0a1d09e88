"""The estimate calls with a base (include/fsehip.h section 2i) through
ctypes, without a device: every argument check that is decided before any
device use (fake non-null pointers, never dereferenced, as in
tests/test_estimate_format.py), fsehip_estimate_base_scratch_bytes against its
formula, the exports, and the calls of section 2g still refusing the diff
kind."""
import ctypes as C

import pytest

import frame_ref as R
import planes_ref as PR
from entropy_coders_amd import _lib
from test_estimate_format import ODD1, ODD2, ODD4, ODD8, OK, es, ih, params, st

MASKS = [m for m in range(1, 24) if not m & 8]  # bits 0, 1, 2 and 4
NEW = ("fsehip_diff_image_histogram", "fsehip_estimate_base_scratch_bytes", "fsehip_estimate_base",
       "fsehip_estimate_choose_base")


def test_exports():
    lib = _lib.load()
    for name in NEW:
        assert name in _lib.EXPORTS and getattr(lib, name) is not None, name


@pytest.mark.parametrize("w", [1, 2, 4, 8])
@pytest.mark.parametrize("n", [0, 1, 16, 17, 4097, 70001, 1 << 30])
def test_base_scratch_bytes(w, n):
    lib = _lib.load()
    stride = PR.stride_of(n)
    image = {0: n * w, 1: 0 if w == 1 else w * stride, 2: w * stride, 4: w * stride}
    for bs in (0, 64, 1040, 65536):
        b = bs or 65536
        for mask in MASKS:
            nb = max([R.n_blocks_of(image[k], b) for k in image if mask >> k & 1 and (k != 1 or w > 1)], default=0)
            assert lib.fsehip_estimate_base_scratch_bytes(n, w, mask, bs) == 1024 * nb, (mask, bs)
            if not mask & 16:
                assert lib.fsehip_estimate_base_scratch_bytes(n, w, mask, bs) == \
                    lib.fsehip_estimate_scratch_bytes(n, w, mask, bs)


def test_base_scratch_bytes_rejects():
    lib = _lib.load()
    for mask in (0, 8, 9, 24, 32, 33, 1 << 31):
        assert lib.fsehip_estimate_base_scratch_bytes(100, 4, mask, 0) == 0, mask
    for w in (0, 3, 5, 16):
        assert lib.fsehip_estimate_base_scratch_bytes(100, w, 16, 0) == 0
    big = (1 << 64) - 1
    assert lib.fsehip_estimate_base_scratch_bytes(big, 1, 16, 0) == 0
    assert lib.fsehip_estimate_base_scratch_bytes(1 << 62, 8, 17, 0) == 0


# ---------------------------------------------------------------- argument checks
def dh(w=4, src=OK, base=OK, n=1000, bs=0, counts=OK):
    return lambda lib: lib.fsehip_diff_image_histogram(w, src, base, n, bs, counts, None)


def eb(p=params(), mask=23, w=4, src=OK, base=OK, n=100000, scratch=OK, cap=1 << 20, est=OK):
    return lambda lib: lib.fsehip_estimate_base(C.byref(p) if p is not None else None, mask, w, src, base, n, scratch,
                                                cap, est, None)


ROWS = []


def row(name, want, call):
    ROWS.append(pytest.param(call, want, id=name))


row("hist-width-3", "UNSUPPORTED", dh(w=3))
row("hist-width-16", "UNSUPPORTED", dh(w=16))
row("hist-width-0", "UNSUPPORTED", dh(w=0))
row("hist-overflow", "UNSUPPORTED", dh(w=8, n=1 << 62))
row("hist-null-src", "BAD_ARG", dh(src=None))
row("hist-null-base", "BAD_ARG", dh(base=None))
row("hist-null-counts", "BAD_ARG", dh(counts=None))
row("hist-src-misaligned-8", "BAD_ARG", dh(w=8, src=ODD4))
row("hist-base-misaligned-8", "BAD_ARG", dh(w=8, base=ODD4))
row("hist-src-misaligned-2", "BAD_ARG", dh(w=2, src=ODD1))
row("hist-base-misaligned-2", "BAD_ARG", dh(w=2, base=ODD1))
row("hist-base-misaligned-4", "BAD_ARG", dh(w=4, base=ODD2))
row("hist-counts-misaligned", "BAD_ARG", dh(counts=ODD2))
row("hist-block-not-16", "BAD_ARG", dh(bs=1000, n=1000))
row("hist-too-many-blocks", "BAD_ARG", dh(w=8, bs=16, n=1 << 34))
row("hist-empty-is-ok", "OK", dh(n=0, src=None, base=None, counts=None))
row("hist-empty-any-block-is-ok", "OK", dh(n=0, bs=1000, src=None, base=None, counts=None))
row("est-null-params", "BAD_ARG", eb(p=None))
row("est-null-est", "BAD_ARG", eb(est=None))
row("est-mask-0", "BAD_ARG", eb(mask=0))
row("est-mask-8", "BAD_ARG", eb(mask=8))
row("est-mask-9", "BAD_ARG", eb(mask=9))
row("est-mask-32", "BAD_ARG", eb(mask=32))
row("est-mask-24", "BAD_ARG", eb(mask=24))
row("est-width-3", "UNSUPPORTED", eb(w=3))
row("est-width-16", "UNSUPPORTED", eb(w=16))
row("est-overflow", "UNSUPPORTED", eb(w=8, n=1 << 62))
row("est-overflow-diff-only", "UNSUPPORTED", eb(mask=16, w=8, n=1 << 62))
row("est-block-above-2-28", "UNSUPPORTED", eb(p=params(bs=(1 << 28) + 16), n=1 << 30, cap=1 << 40))
row("est-block-not-16", "BAD_ARG", eb(p=params(bs=1000)))
row("est-block-not-16-diff-only", "BAD_ARG", eb(mask=16, p=params(bs=1000)))
row("est-nstates-3", "BAD_ARG", eb(p=params(ns=3)))
row("est-ckpt-bad", "BAD_ARG", eb(p=params(ckpt=100)))
row("est-null-src", "BAD_ARG", eb(src=None))
row("est-null-scratch", "BAD_ARG", eb(scratch=None))
row("est-src-misaligned", "BAD_ARG", eb(src=ODD2))
row("est-scratch-misaligned", "BAD_ARG", eb(scratch=ODD8))
row("est-est-misaligned", "BAD_ARG", eb(est=ODD4))
row("est-diff-without-base", "BAD_ARG", eb(base=None))
row("est-diff-only-without-base", "BAD_ARG", eb(mask=16, base=None))
row("est-base-misaligned", "BAD_ARG", eb(base=ODD2))
row("est-base-misaligned-8", "BAD_ARG", eb(w=8, base=ODD4))
row("est-scratch-too-small", "DST_TOO_SMALL", eb(cap=1024 * 7 - 1))  # 400,000 bytes: 7 blocks
row("est-scratch-too-small-diff-only", "DST_TOO_SMALL", eb(mask=16, cap=1024 * 7 - 1))
# the calls of section 2g refuse the diff kind as before
row("old-hist-kind-3", "BAD_ARG", ih(kind=3))
row("old-hist-kind-4", "BAD_ARG", ih(kind=4))
row("old-est-mask-8", "BAD_ARG", es(mask=8))
row("old-est-mask-16", "BAD_ARG", es(mask=16))
row("old-est-mask-23", "BAD_ARG", es(mask=23))


@pytest.mark.parametrize("call,want", ROWS)
def test_argument_checks_come_before_any_device_use(call, want):
    assert st(call(_lib.load())) == want


def test_old_sizes_still_refuse_the_diff_kind():
    lib = _lib.load()
    for kind in (3, 4):
        assert lib.fsehip_estimate_image_bytes(kind, 100, 4) == 0
    for mask in (8, 16, 23):
        assert lib.fsehip_estimate_scratch_bytes(100, 4, mask, 0) == 0
    assert lib.fsehip_estimate_choose(C.byref((C.c_uint64 * 3)(9, 8, 8))) == 1  # the three-entry form


def test_valid_calls_reach_the_device_check():
    """The same calls with valid arguments reach the device check: NO_DEVICE
    without a GPU; with one they would run on fake pointers, so only then
    skipped.  A base is ignored, null or misaligned, when bit 4 is clear, and
    with no elements."""
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present: the calls would run")
    lib = _lib.load()
    for call in (dh(), dh(w=1, src=ODD1, base=ODD2), dh(w=2, src=ODD2, base=ODD4), dh(src=OK, base=OK),
                 eb(), eb(cap=1024 * 7), eb(mask=16), eb(mask=16, w=1, src=ODD1, base=ODD2),
                 eb(mask=7, base=None), eb(mask=7, base=ODD1), eb(mask=5, w=1, src=ODD1, base=None),
                 eb(mask=23, n=0, src=None, base=None, scratch=None, cap=0),
                 eb(mask=16, w=8, n=0, src=None, base=None, scratch=None, cap=0)):
        assert st(call(lib)) == "NO_DEVICE"


def test_python_api_without_gpu():
    from entropy_coders_amd import estimate_choose

    assert estimate_choose({"planes": 5, "delta": 5, "diff": 5}) == "planes"
    assert estimate_choose({"delta": 5, "diff": 5}) == "delta" and estimate_choose({"delta": 5, "diff": 4}) == "diff"
    assert estimate_choose({"diff": 4}) == "diff"
    assert estimate_choose([9, 9, 9, 0, 9]) == "frame" and estimate_choose([9, 9, 9, 0, 8]) == "diff"
    assert estimate_choose([9, 8, 9]) == "planes"
    with pytest.raises(ValueError):
        estimate_choose([_lib.EST_NONE] * 3 + [0, _lib.EST_NONE])
