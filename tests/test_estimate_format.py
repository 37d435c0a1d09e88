"""The size estimate's host side (include/fsehip.h section 2g) through ctypes,
without a device: fsehip_log2q8, fsehip_estimate_block_host and
fsehip_estimate_choose against tests/estimate_ref.py, fsehip_container_kind on
every magic, the sizes, and every argument check that is decided before any
device use (fake non-null pointers, never dereferenced, as in
tests/test_delta_format.py)."""
import ctypes as C

import numpy as np
import pytest

import caller_cases as CC
import delta_ref as DR
import estimate_ref as E
import frame_ref as R
import planes_ref as PR
from entropy_coders_amd import _lib
from oracle import oracle as O

OK = C.c_void_p(4096)
ODD8 = C.c_void_p(4096 + 8)
ODD4 = C.c_void_p(4096 + 4)
ODD2 = C.c_void_p(4096 + 2)
ODD1 = C.c_void_p(4096 + 1)
NONE = E.NONE


def st(rc):
    return _lib.STATUS[rc]


def params(bs=65536, log=0, ckpt=64, lmax=0, ns=2):
    return _lib.FrameParams(bs, log, ckpt, lmax, ns, 0)


def test_log2q8_every_count():
    lib = _lib.load()
    for c in range(1, 32769):
        assert lib.fsehip_log2q8(c) == E.log2q8(c), c
    for c in (0, 32769, 1 << 31, (1 << 32) - 1):
        assert lib.fsehip_log2q8(c) == 0


def test_choose_ties_and_none():
    lib = _lib.load()
    vals = (0, 5, 6, 1 << 40, NONE - 1, NONE)
    for a in vals:
        for b in vals:
            for c in vals:
                arr = (C.c_uint64 * 3)(a, b, c)
                assert lib.fsehip_estimate_choose(C.byref(arr)) == E.choose([a, b, c]), (a, b, c)
    assert lib.fsehip_estimate_choose(C.byref((C.c_uint64 * 3)(7, 7, 7))) == 0
    assert lib.fsehip_estimate_choose(C.byref((C.c_uint64 * 3)(8, 7, 7))) == 1
    assert lib.fsehip_estimate_choose(C.byref((C.c_uint64 * 3)(NONE, NONE, NONE))) == -1
    assert lib.fsehip_estimate_choose(None) == -1


def host_estimate(counts, raw_len, nstates, ckpt, table_log, lmax=0):
    """fsehip_estimate_block_host on the oracle's normalisation of the counts."""
    lib = _lib.load()
    cnt = np.asarray(counts, dtype=np.uint32)
    norm, L, hdr = None, 0, 0
    try:
        h = E.hist_of(cnt, raw_len)
        if raw_len == 0:
            raise O.OracleError(-1)
        nh, _ = O.normalize(h, O.optimal_log2(h) if table_log == 0 else table_log)
        norm = np.asarray(list(nh.norm), dtype=np.int32)
        L, hdr = nh.log2, len(O.header_write(nh))
    except O.OracleError:
        pass
    out = _lib.BlockEstimate()
    p = params(65536, table_log, ckpt, lmax, nstates)
    rc = lib.fsehip_estimate_block_host(cnt.ctypes.data_as(C.c_void_p), raw_len,
                                        norm.ctypes.data_as(C.c_void_p) if norm is not None else None, L, hdr,
                                        C.byref(p), C.byref(out))
    assert rc == 0, st(rc)
    return out.type, out.rec, out.bits, out.table_log


def block_cases():
    rng = np.random.default_rng(0xE57)
    blocks = [b for b in np.split(R.corpus(1000), range(R.BLOCK, 8 * R.BLOCK + 1, R.BLOCK))]
    blocks += [R.corpus(1)[-1:], np.array([0], np.uint8), np.array([3, 3], np.uint8), np.array([1, 2], np.uint8),
               rng.integers(0, 4, 17, dtype=np.uint8), O.generate(0, 0.5, 1, 0, 65536),
               np.minimum(rng.geometric(0.3, 70000), 255).astype(np.uint8)[:65536]]
    return blocks


@pytest.mark.parametrize("nstates", [2, 1])
@pytest.mark.parametrize("ckpt", [0, 64])
@pytest.mark.parametrize("table_log", [0, 9, 12, 13])
def test_block_host_matches_the_reference(nstates, ckpt, table_log):
    for i, blk in enumerate(block_cases()):
        counts = np.bincount(blk, minlength=256)
        want = E.block_estimate(counts, blk.size, nstates=nstates, ckpt=ckpt, table_log=table_log)
        assert host_estimate(counts, blk.size, nstates, ckpt, table_log) == want, i


def test_block_host_caller_counts_and_kernel_class():
    """A caller's count array that normalises on the slow path, and a table
    log above the kernel class (stored RAW)."""
    name, counts, size, tl, log2, label = next(c for c in CC.HIST_CASES if c[0] == "slow_prop_search")
    assert label.startswith("slow") and sum(counts) == size
    want = E.block_estimate(counts, size, nstates=2, ckpt=64, table_log=log2)
    assert want[0] == R.FSE and host_estimate(counts, size, 2, 64, log2) == want
    blk = O.generate(0, 0.155, 1, 0, 65536)
    cnt = np.bincount(blk, minlength=256)
    assert host_estimate(cnt, blk.size, 2, 0, 13, lmax=13)[0] == R.FSE
    assert host_estimate(cnt, blk.size, 2, 0, 13, lmax=12) == (R.RAW, blk.size, 0, 0)
    assert E.block_estimate(cnt, blk.size, table_log=13, max_table_log=12) == (R.RAW, blk.size, 0, 0)


def test_block_host_rejects():
    lib = _lib.load()
    cnt = np.zeros(256, np.uint32)
    cnt[1], cnt[2] = 60, 40
    norm = np.zeros(256, np.int32)
    norm[1], norm[2] = 20, 12
    out = _lib.BlockEstimate()
    cp, npn = cnt.ctypes.data_as(C.c_void_p), norm.ctypes.data_as(C.c_void_p)

    def call(c=cp, n=npn, L=5, p=params(), o=out):
        return st(lib.fsehip_estimate_block_host(c, 100, n, L, 4, C.byref(p) if p is not None else None,
                                                 C.byref(o) if o is not None else None))

    assert call() == "OK" and out.type == R.FSE
    assert call(c=None) == call(p=None) == call(o=None) == "BAD_ARG"
    assert call(p=params(ns=3)) == "BAD_ARG"
    assert call(L=4) == call(L=16) == "BAD_ARG"
    norm[2] = 0  # a byte that occurs has no slot
    assert call() == "BAD_ARG"
    norm[2] = 33  # above 2^5
    assert call() == "BAD_ARG"
    norm[2] = -2
    assert call() == "BAD_ARG"
    assert call(n=None) == "OK" and (out.type, out.rec) == (R.RAW, 100)


def test_container_kind():
    lib = _lib.load()

    def kind(b):
        a = np.frombuffer(bytes(b), dtype=np.uint8) if len(b) else np.zeros(0, np.uint8)
        return lib.fsehip_container_kind(a.ctypes.data_as(C.c_void_p), len(a))

    x = np.arange(100, dtype=np.int32)
    assert kind(R.build_frame(PR.raw_bytes(x), 4096, 128, 2)) == 0
    assert kind(PR.build(x, 4096, 128, 2)) == 1
    assert kind(DR.build(x, 4096, 128, 2)) == 2
    assert kind(b"FSEK" + bytes(28)) == _lib.KIND_SEALED == 3
    assert kind(b"FSEF") == 0 and kind(b"FSEP") == 1 and kind(b"FSED") == 2
    for bad in (b"", b"FSE", b"FSEX", b"fsef", b"\0\0\0\0", b"XSEF1234", b"FSE\0"):
        assert st(kind(bad)) == "BAD_FRAME", bad
    assert st(lib.fsehip_container_kind(None, 4)) == "BAD_ARG"
    assert st(lib.fsehip_container_kind(None, 0)) == "BAD_FRAME"


@pytest.mark.parametrize("w", [1, 2, 4, 8])
@pytest.mark.parametrize("n", [0, 1, 16, 17, 4097, 70001, 1 << 30])
def test_image_and_scratch_bytes(w, n):
    lib = _lib.load()
    stride = PR.stride_of(n)
    want = {0: n * w, 1: 0 if w == 1 else w * stride, 2: w * stride}
    for k in range(3):
        assert lib.fsehip_estimate_image_bytes(k, n, w) == want[k]
    for bs in (0, 64, 1040, 65536):
        b = bs or 65536
        for mask in range(1, 8):
            nb = max([R.n_blocks_of(want[k], b) for k in range(3) if mask >> k & 1 and (k != 1 or w > 1)], default=0)
            assert lib.fsehip_estimate_scratch_bytes(n, w, mask, bs) == 1024 * nb, (mask, bs)


def test_sizes_reject():
    lib = _lib.load()
    for w in (0, 3, 5, 16):
        assert lib.fsehip_estimate_image_bytes(0, 100, w) == 0
        assert lib.fsehip_estimate_scratch_bytes(100, w, 7, 0) == 0
    assert lib.fsehip_estimate_image_bytes(3, 100, 4) == 0
    assert lib.fsehip_estimate_scratch_bytes(100, 4, 0, 0) == lib.fsehip_estimate_scratch_bytes(100, 4, 8, 0) == 0
    big = (1 << 64) - 1
    assert lib.fsehip_estimate_image_bytes(0, big, 2) == lib.fsehip_estimate_image_bytes(2, big, 1) == 0
    assert lib.fsehip_estimate_image_bytes(1, (1 << 62), 8) == 0
    assert lib.fsehip_estimate_scratch_bytes(big, 1, 4, 0) == 0


# ---------------------------------------------------------------- argument checks
def ih(kind=2, w=4, src=OK, n=1000, bs=0, counts=OK):
    return lambda lib: lib.fsehip_image_histogram(kind, w, src, n, bs, counts, None)


def eb(p=params(), counts=OK, n=100000, typ=OK, rec=OK, bits=OK, log=OK, total=OK):
    return lambda lib: lib.fsehip_estimate_blocks(C.byref(p) if p is not None else None, counts, n, typ, rec, bits, log,
                                                  total, None)


def es(p=params(), mask=7, w=4, src=OK, n=100000, scratch=OK, cap=1 << 20, est=OK):
    return lambda lib: lib.fsehip_estimate(C.byref(p) if p is not None else None, mask, w, src, n, scratch, cap, est,
                                           None)


ROWS = []


def row(name, want, call):
    ROWS.append(pytest.param(call, want, id=name))


row("hist-kind-3", "BAD_ARG", ih(kind=3))
row("hist-width-3", "UNSUPPORTED", ih(w=3))
row("hist-width-0", "UNSUPPORTED", ih(w=0))
row("hist-planes-width-1", "UNSUPPORTED", ih(kind=1, w=1))
row("hist-overflow", "UNSUPPORTED", ih(w=8, n=1 << 62))
row("hist-null-src", "BAD_ARG", ih(src=None))
row("hist-null-counts", "BAD_ARG", ih(counts=None))
row("hist-src-misaligned-8", "BAD_ARG", ih(w=8, src=ODD4))
row("hist-src-misaligned-2", "BAD_ARG", ih(w=2, src=ODD1))
row("hist-frame-src-misaligned", "BAD_ARG", ih(kind=0, w=4, src=ODD2))
row("hist-counts-misaligned", "BAD_ARG", ih(counts=ODD2))
row("hist-block-not-16", "BAD_ARG", ih(bs=1000, n=1000))
row("hist-too-many-blocks", "BAD_ARG", ih(w=8, bs=16, n=1 << 34))
row("hist-empty-is-ok", "OK", ih(n=0, src=None, counts=None))
row("blocks-null-params", "BAD_ARG", eb(p=None))
row("blocks-null-total", "BAD_ARG", eb(total=None))
row("blocks-null-counts", "BAD_ARG", eb(counts=None))
row("blocks-counts-misaligned", "BAD_ARG", eb(counts=ODD2))
row("blocks-rec-misaligned", "BAD_ARG", eb(rec=ODD1))
row("blocks-bits-misaligned", "BAD_ARG", eb(bits=ODD2))
row("blocks-total-misaligned", "BAD_ARG", eb(total=ODD4))
row("blocks-nstates-3", "BAD_ARG", eb(p=params(ns=3)))
row("blocks-ckpt-not-power-of-two", "BAD_ARG", eb(p=params(ckpt=48)))
row("blocks-ckpt-too-small", "BAD_ARG", eb(p=params(ckpt=4)))
row("blocks-ckpt-8-one-state", "BAD_ARG", eb(p=params(ckpt=8, ns=1)))
row("blocks-block-not-16", "BAD_ARG", eb(p=params(bs=1000)))
row("blocks-block-above-2-28", "UNSUPPORTED", eb(p=params(bs=(1 << 28) + 16), n=1 << 30))
row("est-null-params", "BAD_ARG", es(p=None))
row("est-null-est", "BAD_ARG", es(est=None))
row("est-mask-0", "BAD_ARG", es(mask=0))
row("est-mask-8", "BAD_ARG", es(mask=8))
row("est-width-3", "UNSUPPORTED", es(w=3))
row("est-overflow", "UNSUPPORTED", es(w=8, n=1 << 62))
row("est-block-above-2-28", "UNSUPPORTED", es(p=params(bs=(1 << 28) + 16), n=1 << 30, cap=1 << 40))
row("est-block-not-16", "BAD_ARG", es(p=params(bs=1000)))
row("est-nstates-3", "BAD_ARG", es(p=params(ns=3)))
row("est-ckpt-bad", "BAD_ARG", es(p=params(ckpt=100)))
row("est-null-src", "BAD_ARG", es(src=None))
row("est-null-scratch", "BAD_ARG", es(scratch=None))
row("est-src-misaligned", "BAD_ARG", es(src=ODD2))
row("est-scratch-misaligned", "BAD_ARG", es(scratch=ODD8))
row("est-est-misaligned", "BAD_ARG", es(est=ODD4))
row("est-scratch-too-small", "DST_TOO_SMALL", es(cap=1024 * 7 - 1))  # 400,000 bytes: 7 blocks


@pytest.mark.parametrize("call,want", ROWS)
def test_argument_checks_come_before_any_device_use(call, want):
    assert st(call(_lib.load())) == want


def test_valid_calls_reach_the_device_check():
    """The same calls with valid arguments reach the device check: NO_DEVICE
    without a GPU; with one they would run on fake pointers, so only then
    skipped."""
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present: the calls would run")
    lib = _lib.load()
    for call in (ih(), ih(kind=0, w=1, src=ODD1), ih(kind=1, w=2, src=ODD2), ih(w=1, src=ODD1), eb(),
                 eb(typ=None, rec=None, bits=None, log=None), eb(n=0, counts=None), es(), es(cap=1024 * 7),
                 es(mask=2, w=1, n=0, src=None, scratch=None, cap=0), es(mask=5, w=1, src=ODD1)):
        assert st(call(lib)) == "NO_DEVICE"


def test_python_api_without_gpu():
    from entropy_coders_amd import FseError, container_kind, estimate_choose, log2q8

    assert log2q8(1) == 0 and log2q8(32768) == 256 * 15 and log2q8(3) == E.log2q8(3)
    with pytest.raises(ValueError):
        log2q8(0)
    assert estimate_choose({"planes": 5, "delta": 5}) == "planes" and estimate_choose([9, 9, 9]) == "frame"
    assert estimate_choose({"frame": 10, "delta": 9}) == "delta"
    with pytest.raises(ValueError):
        estimate_choose({})
    assert container_kind(b"FSEDxxxx") == "delta" and container_kind(np.frombuffer(b"FSEK", np.uint8)) == "sealed"
    with pytest.raises(FseError) as e:
        container_kind(b"nope")
    assert e.value.code == "BAD_FRAME"
