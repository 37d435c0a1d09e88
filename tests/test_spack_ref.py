"""tests/spack_ref.py against itself and against zlib (CPU, no library): the
record's layout byte by byte, build -> parse round trips over pack frames and
versioned packs, and every reject rule of include/fsehip.h section 2l."""
import struct
import zlib

import numpy as np
import pytest

import pack_ref as KR
import spack_ref as SR
import vpack_ref as VR


def members_of(seed=1):
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 1 << 16, 300, dtype=np.uint16)
    b = (a - rng.integers(0, 3, 300).astype(np.uint16)).astype(np.uint16)
    c = np.cumsum(rng.integers(0, 9, 1000)).astype(np.uint32)
    e = np.zeros(0, np.uint64)
    d = rng.integers(0, 256, 77, dtype=np.uint8)
    return [("diff", a, b), ("delta", c, None), ("diff", e, e), ("planes", d, None)]


def test_record_layout():
    members = members_of()
    rec = SR.record(members, True)
    assert len(rec) == SR.record_bytes(4) == 64
    assert rec[:4] == b"FSES" and rec[4:8] == bytes([1, 1, 1, 0])
    assert struct.unpack_from("<II", rec, 8) == (4, 0)
    assert struct.unpack_from("<QI", rec, 16) == (600 + 4000 + 77, 0)
    assert struct.unpack_from("<I", rec, 28)[0] == zlib.crc32(rec[:28])
    tab = [struct.unpack_from("<II", rec, 32 + 8 * m) for m in range(4)]
    assert tab[0] == (zlib.crc32(members[0][1].tobytes()), zlib.crc32(members[0][2].tobytes()))
    assert tab[1] == (zlib.crc32(members[1][1].tobytes()), 0)
    assert tab[2] == (0, 0)  # an empty diff member: no content, no base
    assert tab[3] == (zlib.crc32(members[3][1].tobytes()), 0)
    bare = SR.record(members, False)
    assert bare[6] == 0 and all(struct.unpack_from("<I", bare, 36 + 8 * m)[0] == 0 for m in range(4))
    assert [struct.unpack_from("<I", bare, 32 + 8 * m)[0] for m in range(4)] == [c for c, _ in tab]


@pytest.mark.parametrize("versioned,check_bases", [(True, True), (True, False), (False, False)])
def test_build_parse_round_trip(versioned, check_bases):
    members = members_of(2)
    if not versioned:
        members = [("planes" if k == "diff" else k, a, None) for k, a, _ in members]
    blob = SR.build(members, 4096, 128, 2, versioned=versioned, check_bases=check_bases)
    f, tab, v, inner = SR.parse(blob)
    assert v == versioned and f["flags"] == int(versioned and check_bases) and f["n_members"] == 4
    assert tab == SR.table(members, versioned and check_bases)
    pack = (VR.build(members, 4096, 128, 2) if versioned else
            KR.build([(k, a) for k, a, _ in members], 4096, 128, 2))
    assert inner == pack, "the inner container's bytes are unchanged"
    specs, raws = (VR.decode(inner, [b for _, _, b in members]) if versioned else KR.decode(inner))
    mst, bst = SR.verify(tab, f["flags"], VR.specs_of(members), raws,
                         [VR.raw_bytes(b) if b is not None else b"" for _, _, b in members])
    assert not any(mst) and not any(bst)
    wrong = [VR.raw_bytes(b).copy() if b is not None else b"" for _, _, b in members]
    if versioned:
        wrong[0][5] ^= 1
        mst, bst = SR.verify(tab, f["flags"], VR.specs_of(members), raws, wrong)
        assert bst == ([SR.CHECKSUM, 0, 0, 0] if check_bases else [0, 0, 0, 0])


def test_reject_rules():
    members = members_of(3)
    good = SR.build(members, 4096, 128, 2)
    n = 4
    off = SR.record_bytes(n)
    SR.parse(good)

    def reheader(**kw):
        return SR.header(kw.pop("n", n), kw.pop("content", VR.sums(VR.specs_of(members))[1]), **kw) + good[32:]

    for bad in (b"FSEK" + good[4:], reheader(version=2), reheader(algorithm=2), reheader(flags=3), reheader(spare=1),
                reheader(reserved0=1), reheader(reserved1=1), reheader(header_crc=0), reheader(content=1),
                good[:32] + good[40:],  # a table one entry short: no pack where it should start
                good[:off] + b"FSEF" + good[off + 4:], good[: off + 31]):
        with pytest.raises((SR.SpackError, KR.PackError)):
            SR.parse(bad)
    # n_members that disagrees with the pack's, with a table of that length
    with pytest.raises((SR.SpackError, KR.PackError)):
        SR.parse(SR.header(n + 1, VR.sums(VR.specs_of(members))[1]) + good[32:off] + bytes(8) + good[off:])
    # base CRCs in front of a pack frame
    plain = [("planes" if k == "diff" else k, a, None) for k, a, _ in members]
    pk = SR.build(plain, 4096, 128, 2, versioned=False)
    with pytest.raises(SR.SpackError):
        SR.parse(SR.header(n, VR.sums(VR.specs_of(plain))[1], flags=1) + pk[32:])
