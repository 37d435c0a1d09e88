"""The check record and sealed buffers (include/fsehip.h section 2f) restated
in Python over zlib, tests/frame_ref.py, planes_ref.py and delta_ref.py: a
helper for the check tests, not a test.

  mulmod, xpow8, combine   the CRC-32 combine, written out (no zlib call)
  block_crcs               zlib.crc32 per check block
  header, record           the 32 header bytes; the whole record
  parse                    a record's fields
  seal                     record || container, the container from the refs
  covered, verified_bytes  which check blocks a byte range wholly covers

Nothing here calls the library under test.
"""
import struct
import zlib

import numpy as np

import delta_ref as DR
import frame_ref as R
import planes_ref as PR

MAGIC = b"FSEK"
CHECKSUM, BAD_FRAME = -21, -19
POLY = 0xEDB88320


def mulmod(a, b):
    """a * b mod P, reflected: bit 31 is x^0."""
    p, m = 0, 1 << 31
    while m:
        if a & m:
            p ^= b
        b = (b >> 1) ^ (POLY if b & 1 else 0)
        m >>= 1
    return p


def xpow8(n):
    """x^(8 n) mod P."""
    r, sq = 1 << 31, 1 << 23
    while n:
        if n & 1:
            r = mulmod(r, sq)
        sq = mulmod(sq, sq)
        n >>= 1
    return r


def combine(crc1, crc2, len2):
    """crc(A || B) from crc(A), crc(B), len(B): the init and final XOR cancel."""
    return mulmod(xpow8(len2), crc1) ^ crc2


def n_cb_of(n, check_log):
    return (n + (1 << check_log) - 1) >> check_log


def block_crcs(content, check_log):
    content = bytes(content)
    B = 1 << check_log
    return [zlib.crc32(content[i: i + B]) for i in range(0, len(content), B)]


def header(check_log, n_content, n_cb, content_crc, version=1, algorithm=1, byte7=0, reserved=0, magic=MAGIC,
           header_crc=None):
    h = magic + struct.pack("<BBBBQIII", version, algorithm, check_log, byte7, n_content, n_cb, content_crc, reserved)
    return h + struct.pack("<I", zlib.crc32(h) if header_crc is None else header_crc)


def record(content, check_log=16):
    content = bytes(content)
    crcs = block_crcs(content, check_log)
    whole = 0
    for i, c in enumerate(crcs):  # the combine, not a second pass
        whole = combine(whole, c, min(1 << check_log, len(content) - (i << check_log)))
    assert whole == zlib.crc32(content)
    return header(check_log, len(content), len(crcs), whole) + struct.pack(f"<{len(crcs)}I", *crcs)


def record_bytes(n, check_log=16):
    return 32 + 4 * n_cb_of(n, check_log)


def parse(rec):
    rec = bytes(rec)
    assert rec[:4] == MAGIC
    version, algorithm, check_log, byte7, n, n_cb, crc, reserved, hcrc = struct.unpack("<BBBBQIIII", rec[4:32])
    return {"version": version, "algorithm": algorithm, "check_log": check_log, "n_content": n, "n_cb": n_cb,
            "content_crc": crc, "header_crc": hcrc, "table": list(struct.unpack(f"<{n_cb}I", rec[32: 32 + 4 * n_cb]))}


def refresh_header_crc(rec):
    """The record with header_crc recomputed over whatever bytes 0..27 now hold."""
    rec = bytes(rec)
    return rec[:28] + struct.pack("<I", zlib.crc32(rec[:28])) + rec[32:]


def seal(elems, kind, block_size, ckpt, nstates, check_log=16, table_log=0):
    """record || container of an array: kind 'frame' (bytes), 'planes', 'delta'."""
    a = np.ascontiguousarray(elems).reshape(-1)
    raw = PR.raw_bytes(a)
    if kind == "frame":
        inner = R.build_frame(raw, block_size, ckpt, nstates, table_log)
    elif kind == "planes":
        inner = PR.build(a, block_size, ckpt, nstates, table_log)
    else:
        inner = DR.build(a, block_size, ckpt, nstates, table_log)
    return record(raw.tobytes(), check_log) + bytes(inner)


def covered(n, check_log, src_off, length):
    """The check blocks wholly inside [src_off, src_off + length), byte by
    byte: a block counts when every one of its content bytes is in the range."""
    B = 1 << check_log
    out = []
    for b in range(n_cb_of(n, check_log)):
        lo, hi = b * B, min((b + 1) * B, n)
        if length and src_off <= lo and hi <= src_off + length:
            out.append(b)
    return out


def verified_bytes(n, check_log, ranges):
    B = 1 << check_log
    return sum(min((b + 1) * B, n) - b * B for s, ln, *_ in ranges for b in covered(n, check_log, s, ln))
