"""The versioned pack (include/fsehip.h section 2k) restated in numpy over
tests/pack_ref.py, tests/diff_ref.py, tests/delta_ref.py and
tests/frame_ref.py: a helper for the versioned-pack tests, not a test.

A member is (kind, array, base | None): kind "planes", "delta" or "diff", a
1-D array of 1-, 2-, 4- or 8-byte items, and for "diff" a base of the same
item size and count (ignored for the other kinds).  A spec is what the table
stores of it: (kind, w, n).  The layout is the pack frame's; only the magic
and the kind list differ.

  normalise      arrays, kinds, bases -> members
  specs_of       members -> specs
  image          members -> the pack image (plane-major from the top byte)
  unimage        image, specs, bases -> the members' raw bytes
  header         specs -> the 32 + 16 n head bytes
  build          members -> versioned pack, the inner frame from frame_ref.build_frame
  parse          versioned pack -> (specs, the inner frame's bytes)
  decode         versioned pack, bases -> (specs, the members' raw bytes)
  table_rows     the member lists of the size table in DESIGN.md section 5 "Versioned pack"

Nothing here calls the library under test.
"""
import struct

import numpy as np

import delta_ref as DR
import diff_ref as FR
import frame_ref as R
import pack_ref as KR
import planes_ref as PR

MAGIC = b"FSEV"
KIND = {"planes": 1, "delta": 2, "diff": 4}
KIND_NAME = {v: k for k, v in KIND.items()}
WIDTHS = KR.WIDTHS
MAX_MEMBERS = KR.MAX_MEMBERS

stride_of = KR.stride_of
raw_bytes = KR.raw_bytes
sums = KR.sums
plane_offsets = KR.plane_offsets
bound = KR.bound
PackError = KR.PackError


def normalise(members, kinds=None, bases=None):
    """[(kind, flat array, flat base | None)] of (kind, array, base) triples, or of a list of arrays
    with kinds=None / a name / a list and bases=None / a list (default kind: "diff" where a base is given)."""
    flat = lambda a: None if a is None else np.ascontiguousarray(a).reshape(-1)  # noqa: E731
    if kinds is None and bases is None and members and isinstance(members[0], tuple):
        out = [(k, flat(a), flat(b)) for k, a, b in members]
    else:
        bases = [None] * len(members) if bases is None else list(bases)
        if kinds is None:
            kinds = ["planes" if b is None else "diff" for b in bases]
        names = [kinds] * len(members) if isinstance(kinds, str) else list(kinds)
        assert len(names) == len(members) == len(bases)
        out = [(k, flat(a), flat(b)) for k, a, b in zip(names, members, bases)]
    for k, a, b in out:
        assert k in KIND
        if k == "diff":
            assert b is not None and b.dtype.itemsize == a.dtype.itemsize and b.size == a.size
    return out


def specs_of(members):
    return [(k, a.dtype.itemsize, a.size) for k, a, _ in members]


def member_planes(kind, raw, w, base_raw=None):
    """The (w, stride) planes of one member's raw bytes."""
    if kind != "diff":
        return KR.member_planes(kind, raw, w)
    return FR.image(raw, base_raw, w).reshape(w, stride_of(np.asarray(raw).size // w))


def image(members):
    members = normalise(members)
    specs = specs_of(members)
    img = np.zeros(sums(specs)[0], dtype=np.uint8)
    for (kind, a, b), (_, w, n), o in zip(members, specs, plane_offsets(specs)):
        planes = member_planes(kind, raw_bytes(a), w, None if b is None else raw_bytes(b))
        for k in range(w):
            img[o[k]: o[k] + stride_of(n)] = planes[k]
    return img


def unimage(img, specs, bases=None):
    """The members' raw bytes (uint8 arrays) of a versioned pack's image; bases[m]: a diff member's base array."""
    img = np.asarray(img, dtype=np.uint8)
    assert img.size == sums(specs)[0]
    out = []
    for m, ((kind, w, n), o) in enumerate(zip(specs, plane_offsets(specs))):
        flat = np.stack([img[o[k]: o[k] + stride_of(n)] for k in range(w)]).reshape(-1)
        if kind == "diff":
            out.append(FR.unimage(flat, raw_bytes(np.ascontiguousarray(bases[m]).reshape(-1)), w, n))
        elif kind == "delta":
            out.append(DR.unimage(flat, w, n))
        else:
            out.append(flat[:n].copy() if w == 1 else PR.unimage(flat, w, n))
    return out


def header(specs, version=1, image_bytes=None, content_bytes=None, magic=MAGIC, n_members=None):
    img, content = sums(specs)
    head = magic + struct.pack("<B3xI4xQQ", version, len(specs) if n_members is None else n_members,
                               img if image_bytes is None else image_bytes,
                               content if content_bytes is None else content_bytes)
    return head + b"".join(struct.pack("<BB6xQ", KIND.get(k, k), w, n) for k, w, n in specs)


def build(members, block_size, ckpt, nstates, table_log=0, sidecars=None, kinds=None, bases=None):
    """The versioned pack of a list of members."""
    members = normalise(members, kinds, bases)
    return header(specs_of(members)) + R.build_frame(image(members), block_size, ckpt, nstates, table_log,
                                                     sidecars=sidecars)


def parse(buf):
    """(specs, inner frame bytes) of a versioned pack; PackError for every rule of the format."""
    buf = bytes(buf)
    if len(buf) < 32 or buf[:4] != MAGIC:
        raise PackError("not a versioned pack")
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


def decode(buf, bases=None):
    """(specs, the members' raw bytes) of a versioned pack against the bases of its diff members."""
    specs, inner = parse(buf)
    return specs, unimage(np.frombuffer(R.decode_frame(inner), dtype=np.uint8), specs, bases)


# ---------------------------------------------------------------- the size table
def table_rows(seed=7):
    """The member lists of the size table in DESIGN.md section 5 "Versioned
    pack": name -> (new arrays, base arrays).  Drawn in this order from one
    torch generator: row by row, first every member's fp32 master (randn *
    0.02, a weight's scale, for the lists of pack_ref.table_rows), then every
    member's noise; the base is the master in the member's format, the new
    tensor master + step * noise in that format."""
    import torch

    g = torch.Generator().manual_seed(seed)

    def randn(n, scale=1.0):
        return (torch.randn(n, generator=g) * scale).numpy()

    bf16 = KR.bf16
    f32 = lambda x: np.ascontiguousarray(x, dtype=np.float32).view(np.int32)  # noqa: E731
    lists = {
        "40 x 256 bf16": [(256, 0.02, bf16)] * 40,
        "24 x 1024 bf16 + 8 x 300 fp32": [(1024, 0.02, bf16)] * 24 + [(300, 0.02, f32)] * 8,
        "4 x 70000 bf16 + 16 x 100 bf16": [(70000, 0.02, bf16)] * 4 + [(100, 0.02, bf16)] * 16,
    }
    rows = {}
    for name, steps in (("40 x 256 bf16", (1e-4,)), ("24 x 1024 bf16 + 8 x 300 fp32", (1e-4, 1e-5)),
                        ("4 x 70000 bf16 + 16 x 100 bf16", (1e-4, 1e-5))):
        for step in steps:
            masters = [randn(n, scale) for n, scale, _ in lists[name]]
            noise = [randn(n) for n, _, _ in lists[name]]
            new = [fmt(m + np.float32(step) * z) for (_, _, fmt), m, z in zip(lists[name], masters, noise)]
            base = [fmt(m) for (_, _, fmt), m in zip(lists[name], masters)]
            rows[f"{name}, step {step:g}"] = (new, base)
    return rows
