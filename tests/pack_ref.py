"""The pack frame (include/fsehip.h section 2j) restated in numpy over
tests/planes_ref.py, tests/delta_ref.py and tests/frame_ref.py: a helper for
the pack tests, not a test.

A member is (kind, array): kind "planes" or "delta", a 1-D array of 1-, 2-,
4- or 8-byte items.  A spec is what the table stores of it: (kind, w, n).

  specs_of       members -> specs
  plane_offsets  specs -> per member, the image offset of each byte plane
  image          members -> the pack image (plane-major from the top byte)
  unimage        image, specs -> the members' raw bytes
  header         specs -> the 32 + 16 n head bytes
  build          members -> pack frame, the inner frame from frame_ref.build_frame
  parse          pack frame -> (specs, the inner frame's bytes)
  decode         pack frame -> (specs, the members' raw bytes)

Nothing here calls the library under test.
"""
import struct

import numpy as np

import delta_ref as DR
import frame_ref as R
import planes_ref as PR

MAGIC = b"FSEM"
KIND = {"planes": 1, "delta": 2}
KIND_NAME = {v: k for k, v in KIND.items()}
WIDTHS = (1, 2, 4, 8)
MAX_MEMBERS = 1 << 20

stride_of = PR.stride_of
raw_bytes = PR.raw_bytes


class PackError(Exception):
    pass


def normalise(members, kinds=None):
    """[(kind, flat array)] of a list of arrays and kinds=None / a name / a list, or of (kind, array) pairs."""
    if kinds is None and members and isinstance(members[0], tuple):
        return [(k, np.ascontiguousarray(a).reshape(-1)) for k, a in members]
    names = ["planes"] * len(members) if kinds is None else [kinds] * len(members) if isinstance(kinds, str) else kinds
    assert len(names) == len(members)
    return [(k, np.ascontiguousarray(a).reshape(-1)) for k, a in zip(names, members)]


def specs_of(members):
    return [(k, a.dtype.itemsize, a.size) for k, a in members]


def sums(specs):
    """(image_bytes, content_bytes)."""
    return sum(w * stride_of(n) for _, w, n in specs), sum(w * n for _, w, n in specs)


def plane_offsets(specs):
    """off[m][k]: where byte k of member m's elements lies in the image."""
    off = [[None] * w for _, w, _ in specs]
    at = 0
    for j in range(8):  # segment j: plane w - 1 - j of every member with w > j, in member order
        for m, (_, w, n) in enumerate(specs):
            if w > j:
                off[m][w - 1 - j] = at
                at += stride_of(n)
    return off


def member_planes(kind, raw, w):
    """The (w, stride) planes of one member's raw bytes."""
    raw = np.asarray(raw, dtype=np.uint8)
    n = raw.size // w
    if kind == "delta":
        return DR.image(raw, w).reshape(w, stride_of(n))
    assert kind == "planes"
    if w == 1:  # the bytes themselves
        out = np.zeros((1, stride_of(n)), dtype=np.uint8)
        out[0, :n] = raw
        return out
    return PR.image(raw, w).reshape(w, stride_of(n))


def image(members):
    members = normalise(members)
    specs = specs_of(members)
    off = plane_offsets(specs)
    img = np.zeros(sums(specs)[0], dtype=np.uint8)
    for (kind, a), (_, w, n), o in zip(members, specs, off):
        planes = member_planes(kind, raw_bytes(a), w)
        for k in range(w):
            img[o[k]: o[k] + stride_of(n)] = planes[k]
    return img


def unimage(img, specs):
    """The members' raw bytes (uint8 arrays) of a pack image."""
    img = np.asarray(img, dtype=np.uint8)
    assert img.size == sums(specs)[0]
    out = []
    for (kind, w, n), o in zip(specs, plane_offsets(specs)):
        planes = np.stack([img[o[k]: o[k] + stride_of(n)] for k in range(w)])
        flat = planes.reshape(-1)
        if kind == "delta":
            out.append(DR.unimage(flat, w, n))
        elif w == 1:
            out.append(flat[:n].copy())
        else:
            out.append(PR.unimage(flat, w, n))
    return out


def header(specs, version=1, image_bytes=None, content_bytes=None, magic=MAGIC, n_members=None):
    img, content = sums(specs)
    head = magic + struct.pack("<B3xI4xQQ", version, len(specs) if n_members is None else n_members,
                               img if image_bytes is None else image_bytes,
                               content if content_bytes is None else content_bytes)
    return head + b"".join(struct.pack("<BB6xQ", KIND[k], w, n) for k, w, n in specs)


def bound(specs, block_size):
    return 32 + 16 * len(specs) + R.bound(sums(specs)[0], block_size)


def build(members, block_size, ckpt, nstates, table_log=0, sidecars=None, kinds=None):
    """The pack frame of a list of members."""
    members = normalise(members, kinds)
    return header(specs_of(members)) + R.build_frame(image(members), block_size, ckpt, nstates, table_log,
                                                     sidecars=sidecars)


def parse(buf):
    """(specs, inner frame bytes) of a pack frame; PackError for every rule of the format."""
    buf = bytes(buf)
    if len(buf) < 32 or buf[:4] != MAGIC:
        raise PackError("not a pack")
    version, r0, n, r1, img, content = struct.unpack("<B3sI4sQQ", buf[4:32])
    if version != 1 or any(r0) or any(r1) or n > MAX_MEMBERS:
        raise PackError("bad header")
    if len(buf) < 32 + 16 * n + 32:
        raise PackError("truncated table")
    specs = []
    for m in range(n):
        kind, w, r, cnt = struct.unpack_from("<BB6sQ", buf, 32 + 16 * m)
        if kind not in KIND_NAME or w not in WIDTHS or any(r):
            raise PackError(f"member {m}")
        specs.append((KIND_NAME[kind], w, cnt))
    if any(n_ > (1 << 64) - 16 for _, _, n_ in specs) or sums(specs)[0] >= 1 << 64 or sums(specs) != (img, content):
        raise PackError("sums")
    inner = buf[32 + 16 * n:]
    if inner[:4] != R.MAGIC or struct.unpack_from("<Q", inner, 16)[0] != img:
        raise PackError("inner frame")
    return specs, inner


def decode(buf):
    """(specs, the members' raw bytes) of a pack frame."""
    specs, inner = parse(buf)
    return specs, unimage(np.frombuffer(R.decode_frame(inner), dtype=np.uint8), specs)


# ---------------------------------------------------------------- the size table
def bf16(x):
    """float32 array -> its bfloat16 bits (round to nearest even), int16."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16).view(np.int16)


def table_rows(seed=3):
    """The member lists of the size table in DESIGN.md section 5 "Pack", drawn
    in this order from one torch generator: name -> list of arrays."""
    import torch

    g = torch.Generator().manual_seed(seed)

    def randn(n, scale=1.0):
        return (torch.randn(n, generator=g) * scale).numpy()

    rows = {}
    rows["40 x 256 bf16"] = [bf16(randn(256, 0.02)) for _ in range(40)]
    rows["24 x 1024 bf16 + 8 x 300 fp32"] = ([bf16(randn(1024)) for _ in range(24)]
                                             + [randn(300, 0.01).astype(np.float32) for _ in range(8)])
    rows["4 x 70000 bf16 + 16 x 100 bf16"] = ([bf16(randn(70000)) for _ in range(4)]
                                              + [bf16(randn(100)) for _ in range(16)])
    return rows
