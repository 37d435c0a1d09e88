"""The member check record and the sealed pack (include/fsehip.h section 2l)
restated with zlib.crc32 over tests/pack_ref.py and tests/vpack_ref.py: a
helper for the sealed-pack tests, not a test.

A member is vpack_ref's (kind, array, base | None).  The record is 32 header
bytes and 8 table bytes per member; a sealed pack is the record followed by
the unchanged pack frame ("FSEM", no bases) or versioned pack ("FSEV").

  header      n_members, content_bytes, flags -> the 32 header bytes
  table       members, with_bases -> [(content_crc, base_crc)]
  record      members, with_bases -> header + table
  build       members -> sealed pack, the pack from pack_ref.build / vpack_ref.build
  parse       sealed pack -> (fields, table, versioned, the pack's bytes)
  verify      table, raws, base raws -> (member statuses, base statuses)

Nothing here calls the library under test.
"""
import struct
import zlib

import numpy as np

import pack_ref as KR
import vpack_ref as VR

MAGIC = b"FSES"
CRC32 = 1
BASES = 1  # flags bit 0
OK, CHECKSUM, BAD_FRAME = 0, -21, -19
MAX_MEMBERS = KR.MAX_MEMBERS


class SpackError(Exception):
    pass


def record_bytes(n):
    return 32 + 8 * n


def header(n_members, content_bytes, flags=0, version=1, algorithm=CRC32, spare=0, reserved0=0, reserved1=0,
           magic=MAGIC, header_crc=None):
    h = magic + struct.pack("<BBBBIIQI", version, algorithm, flags, spare, n_members, reserved0, content_bytes,
                            reserved1)
    assert len(h) == 28
    return h + struct.pack("<I", zlib.crc32(h) if header_crc is None else header_crc)


def crc_of(a):
    raw = VR.raw_bytes(np.ascontiguousarray(a).reshape(-1)).tobytes()
    return zlib.crc32(raw) if raw else 0


def table(members, with_bases):
    members = VR.normalise(members)
    out = []
    for kind, a, b in members:
        based = with_bases and kind == "diff" and a.size
        out.append((crc_of(a), crc_of(b) if based else 0))
    return out


def record(members, with_bases):
    members = VR.normalise(members)
    content = VR.sums(VR.specs_of(members))[1]
    return header(len(members), content, BASES if with_bases else 0) + b"".join(
        struct.pack("<II", c, b) for c, b in table(members, with_bases))


def build(members, block_size, ckpt, nstates, table_log=0, sidecars=None, versioned=True, check_bases=True):
    """The sealed pack of a list of (kind, array, base | None); versioned False: the pack frame, no diff member."""
    members = VR.normalise(members)
    if versioned:
        pack = VR.build(members, block_size, ckpt, nstates, table_log, sidecars=sidecars)
    else:
        assert all(k != "diff" for k, _, _ in members)
        pack = KR.build([(k, a) for k, a, _ in members], block_size, ckpt, nstates, table_log, sidecars=sidecars)
    return record(members, bool(versioned and check_bases)) + pack


def parse_header(hdr):
    """The fields of 32 header bytes; SpackError for every rule of the format."""
    hdr = bytes(hdr)
    if len(hdr) < 32 or hdr[:4] != MAGIC:
        raise SpackError("not a member check record")
    version, algorithm, flags, spare, n, r0, content, r1, crc = struct.unpack("<BBBBIIQII", hdr[4:32])
    if version != 1 or algorithm != CRC32 or flags & ~BASES or spare or r0 or r1 or n > MAX_MEMBERS:
        raise SpackError("bad header")
    if crc != zlib.crc32(hdr[:28]):
        raise SpackError("header crc")
    return {"version": version, "algorithm": algorithm, "flags": flags, "n_members": n, "content_bytes": content,
            "header_crc": crc}


def parse(buf):
    """(fields, [(content_crc, base_crc)], versioned, the pack's bytes) of a sealed pack."""
    buf = bytes(buf)
    f = parse_header(buf[:32])
    off = record_bytes(f["n_members"])
    if len(buf) < off + 32:
        raise SpackError("truncated")
    tab = [struct.unpack_from("<II", buf, 32 + 8 * m) for m in range(f["n_members"])]
    inner = buf[off:]
    if inner[:4] not in (KR.MAGIC, VR.MAGIC):
        raise SpackError("no pack behind the record")
    versioned = inner[:4] == VR.MAGIC
    if f["flags"] & BASES and not versioned:
        raise SpackError("base CRCs in front of a pack frame")
    n, = struct.unpack_from("<I", inner, 8)
    content, = struct.unpack_from("<Q", inner, 24)
    if n != f["n_members"] or content != f["content_bytes"]:
        raise SpackError("record and pack disagree")
    (VR if versioned else KR).parse(inner)  # the pack's own rules
    return f, tab, versioned, inner


def verify(tab, flags, specs, raws, base_raws=None):
    """(member statuses, base statuses) of raw bytes against a table."""
    mst, bst = [], []
    for m, ((kind, w, n), (c, b)) in enumerate(zip(specs, tab)):
        raw = bytes(raws[m])
        mst.append(OK if (zlib.crc32(raw) if raw else 0) == c else CHECKSUM)
        if flags & BASES:
            braw = bytes(base_raws[m]) if kind == "diff" and n else b""
            bst.append(OK if (zlib.crc32(braw) if braw else 0) == b else CHECKSUM)
        else:
            bst.append(OK)
    return mst, bst
