"""The frame's host side without a GPU: header parsing and the bound
(csrc/fse_frame.cpp) against tests/frame_ref.py, the call-level errors of
fsehip_frame_compress / fsehip_frame_decompress before any device work, and
the reference itself round-tripping the corpora on the oracle."""
import ctypes as C
import struct

import numpy as np
import pytest

import frame_ref as R
from entropy_coders_amd import _lib

BLOCK, CKPT = R.BLOCK, R.CKPT


def read_header(data):
    a = np.frombuffer(bytes(data), dtype=np.uint8)
    info = _lib.FrameInfo()
    rc = _lib.load().fsehip_frame_read_header(a.ctypes.data_as(C.c_void_p), len(a), C.byref(info))
    return _lib.STATUS[rc], info


GOOD = [  # (nstates, max_table_log, block_size, ckpt, n_total)
    (2, 11, 4096, 128, 10 * 4096 + 1000), (1, 11, 4096, 16, 4096), (2, 15, 65536, 0, 1 << 33), (2, 11, 65536, 8, 0),
    (1, 12, 1000, 0, 999), (2, 13, 1 << 28, 128, (1 << 28) + 1), (2, 11, 7, 0, 7),
]


@pytest.mark.parametrize("nstates,mlog,bs,ckpt,n_total", GOOD)
def test_header_round_trip(nstates, mlog, bs, ckpt, n_total):
    hdr = R.header(nstates, mlog, bs, ckpt, n_total)
    assert len(hdr) == 32
    code, info = read_header(hdr + b"\xEE" * 5)  # only the first 32 bytes count
    assert code == "OK"
    nb = R.n_blocks_of(n_total, bs)
    assert (info.version, info.nstates, info.max_table_log, info.flags) == (1, nstates, mlog, 1 if ckpt else 0)
    assert (info.block_size, info.ckpt_interval, info.n_total, info.n_blocks) == (bs, ckpt, n_total, nb)
    assert info.records_off == 32 + 4 * nb and info.reserved == 0
    out = (C.c_uint8 * 32)()
    assert _lib.load().fsehip_frame_write_header(C.byref(info), out) == 0
    assert bytes(out) == hdr


BAD = {
    "magic": dict(magic=b"FSEG"),
    "version 0": dict(version=0),
    "version 2": dict(version=2),
    "nstates 0": dict(nstates=0),
    "nstates 3": dict(nstates=3),
    "max_table_log 10": dict(max_table_log=10),
    "max_table_log 16": dict(max_table_log=16),
    "flag bit 1": dict(flags=3),
    "flags clear with an interval": dict(flags=0),
    "block_size 0": dict(block_size=0, n_blocks=0),
    "block_size above 2^28": dict(block_size=(1 << 28) + 16),
    "block_size not a multiple of 16": dict(block_size=4100),
    "interval not a power of two": dict(ckpt=96),
    "interval below 8": dict(ckpt=4),
    "interval 0 with the flag": dict(ckpt=0, flags=1),
    "n_blocks short": dict(n_blocks=10),
    "n_blocks long": dict(n_blocks=12),
    "reserved": dict(reserved=1),
}


@pytest.mark.parametrize("what", sorted(BAD))
def test_header_single_field_corruption(what):
    f = dict(nstates=2, max_table_log=11, block_size=4096, ckpt=128, n_total=10 * 4096 + 1000)
    assert read_header(R.header(**f))[0] == "OK"
    f.update(BAD[what])
    assert read_header(R.header(**f))[0] == "BAD_FRAME", what
    out = (C.c_uint8 * 32)()
    info = _lib.FrameInfo(f.get("version", 1), f["nstates"], f["max_table_log"], f.get("flags", 1 if f["ckpt"] else 0),
                          f["block_size"], f["ckpt"],
                          f.get("n_blocks", R.n_blocks_of(f["n_total"], f["block_size"] or 1)), f.get("reserved", 0),
                          f["n_total"], 0)
    if what != "magic":  # the writer refuses the same fields
        assert _lib.STATUS[_lib.load().fsehip_frame_write_header(C.byref(info), out)] == "BAD_ARG"


def test_header_one_state_interval_floor():
    assert read_header(R.header(1, 11, 4096, 8, 4096))[0] == "BAD_FRAME"  # 1-state: >= 16
    assert read_header(R.header(1, 11, 4096, 16, 4096))[0] == "OK"
    assert read_header(R.header(2, 11, 4096, 8, 4096))[0] == "OK"


def test_header_short_lengths():
    hdr = R.header(2, 11, 4096, 128, 5000)
    for n in range(32):
        assert read_header(hdr[:n])[0] == "BAD_FRAME", n
    assert read_header(hdr)[0] == "OK"


def test_frame_bound():
    lib = _lib.load()
    bs = BLOCK
    for n in (0, 1, bs - 1, bs, bs + 1, 10 * bs + 1000):
        assert lib.fsehip_frame_bound(n, bs) == 32 + 4 * -(-n // bs) + n == R.bound(n, bs)
    assert lib.fsehip_frame_bound(65537, 0) == 32 + 4 * 2 + 65537  # 0 = the default 64 KiB block


def _compress(p, src=4096, n=10 * BLOCK, frame=8192, cap=None, flen=16384, res=32768):
    cap = R.bound(n, p.block_size or 65536) if cap is None else cap
    v = C.c_void_p
    return _lib.STATUS[_lib.load().fsehip_frame_compress(C.byref(p), v(src), n, v(frame), cap, v(flen), v(res), None)]


def _decompress(info, frame=8192, frame_len=1 << 20, out=4096, cap=None, st=16384, res=32768):
    cap = info.n_total if cap is None else cap
    v = C.c_void_p
    return _lib.STATUS[_lib.load().fsehip_frame_decompress(C.byref(info), 0, v(frame), frame_len, v(out), cap, v(st),
                                                            v(res), None)]


def _info(nstates=2, mlog=11, bs=BLOCK, ckpt=CKPT, n_total=10 * BLOCK):
    code, info = read_header(R.header(nstates, mlog, bs, ckpt, n_total))
    assert code == "OK"
    return info


def test_call_level_errors_before_any_gpu_work():
    """Fake pointers: every one of these returns before the device is touched
    (the tests/test_abi.py pattern)."""
    FP = _lib.FrameParams
    assert _compress(FP(BLOCK, 0, CKPT, 11, 2, 0), cap=R.bound(10 * BLOCK, BLOCK) - 1) == "DST_TOO_SMALL"
    assert _compress(FP(BLOCK, 0, CKPT, 11, 3, 0)) == "BAD_ARG"
    assert _compress(FP(BLOCK, 0, 96, 11, 2, 0)) == "BAD_ARG"    # not a power of two
    assert _compress(FP(BLOCK, 0, 4, 11, 2, 0)) == "BAD_ARG"     # below 8
    assert _compress(FP(BLOCK, 0, 8, 11, 1, 0)) == "BAD_ARG"     # 1-state: below 16
    assert _compress(FP(BLOCK, 0, CKPT, 11, 2, 0), src=4096 + 8) == "BAD_ARG"  # misaligned d_src
    assert _compress(FP(4100, 0, CKPT, 11, 2, 0), n=3 * 4100) == "BAD_ARG"     # blocks not a multiple of 16
    assert _compress(FP(1 << 29, 0, CKPT, 11, 2, 0), n=1 << 29) == "UNSUPPORTED"
    assert _compress(FP(BLOCK, 0, CKPT, 11, 2, 0), frame=0) == "BAD_ARG"
    assert _compress(FP(BLOCK, 0, CKPT, 11, 2, 0), res=0) == "BAD_ARG"

    assert _decompress(_info(), out=4096 + 8) == "BAD_ARG"  # misaligned d_out
    assert _decompress(_info(), cap=10 * BLOCK - 1) == "DST_TOO_SMALL"
    assert _decompress(_info(), res=0) == "BAD_ARG"
    for field, value in (("nstates", 3), ("ckpt_interval", 96), ("n_blocks", 9), ("reserved", 1), ("version", 2)):
        info = _info()
        setattr(info, field, value)
        assert _decompress(info) == "BAD_ARG", field
    info = _info()
    info.block_size = 1 << 29
    assert _decompress(info) == "UNSUPPORTED"


def test_valid_arguments_need_a_device():
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    assert _compress(_lib.FrameParams(BLOCK, 0, CKPT, 11, 2, 0)) == "NO_DEVICE"
    assert _compress(_lib.FrameParams(BLOCK, 0, 0, 0, 0, 0), src=0, n=0) == "NO_DEVICE"  # the empty input is valid
    assert _decompress(_info()) == "NO_DEVICE"
    assert _decompress(_info(n_total=0), out=0, st=0) == "NO_DEVICE"


def test_python_api_is_exported():
    import entropy_coders_amd as E

    assert _lib.STATUS[-19] == "BAD_FRAME"
    for name in ("frame_bound", "compress_frame", "compress_frame_into", "decompress_frame", "decompress_frame_into",
                 "frame_info"):
        assert callable(getattr(E.BlockCodec, name)), name
    assert callable(E.frame_compress) and callable(E.frame_decompress)
    info = E.BlockCodec.frame_info(R.header(2, 11, 4096, 128, 5000))
    assert (info.n_total, info.n_blocks, info.records_off) == (5000, 2, 40)
    with pytest.raises(E.FseError) as e:
        E.BlockCodec.frame_info(b"not a frame, but long enough to hold a header")
    assert e.value.code == "BAD_FRAME"


# ---------------------------------------------------------------- the reference on the oracle
@pytest.fixture(scope="module")
def corpora():
    return {t: R.corpus(t) for t in (1000, 1)}


def test_corpus_condition(corpora):
    """All three record types occur, block by block as the corpus intends, and the 1-byte tail is RAW."""
    for tail, raw in corpora.items():
        for nstates in (2, 1):
            info, directory, _ = R.split_frame(R.build_frame(raw, BLOCK, CKPT, nstates))
            types = [t for t, _ in directory]
            assert types[:8] == [R.FSE, R.FSE, R.RAW, R.RAW, R.RLE, R.FSE, R.FSE, R.RAW], (tail, nstates, types)
            assert directory[4] == (R.RLE, 1)
            if tail == 1000:
                assert types[8] == R.FSE
            else:
                assert directory[8] == (R.RAW, 1)


@pytest.mark.parametrize("nstates", [2, 1])
@pytest.mark.parametrize("ckpt", [CKPT, 0])
@pytest.mark.parametrize("tail", [1000, 1])
def test_reference_round_trip(corpora, tail, ckpt, nstates):
    raw = corpora[tail]
    frame = R.build_frame(raw, BLOCK, ckpt, nstates)
    assert len(frame) <= R.bound(len(raw), BLOCK)
    code, info = read_header(frame)
    assert code == "OK" and info.n_total == len(raw) and info.flags == (1 if ckpt else 0)
    parsed, directory, records = R.split_frame(frame)
    assert parsed["records_off"] == info.records_off
    for b, ((typ, ln), (side, data)) in enumerate(zip(directory, records)):
        n = R.raw_len(len(raw), BLOCK, b)
        assert len(data) == ln
        assert len(side) == (R.spb_of(n, ckpt, nstates) if typ == R.FSE else 0)
        assert len(data) + 8 * len(side) <= n  # no record is larger than its block (FSE: strictly smaller)
    assert R.decode_frame(frame) == raw.tobytes()


def test_reference_rejects_wrong_lengths(corpora):
    frame = R.build_frame(corpora[1000], BLOCK, CKPT, 2)
    for bad in (frame[:-1], frame + b"\x00", frame[:40]):
        with pytest.raises(R.FrameError):
            R.split_frame(bad)
    assert struct.unpack_from("<I", frame, 24)[0] == 9
